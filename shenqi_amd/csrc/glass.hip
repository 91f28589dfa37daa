/* glass.hip — glass making on the device for one rank: glass_evolve (libgenic/glass.cpp:76-147) with glass_force, _prepare, the
 * transfers and the readouts (glass.cpp:184-360), glass_stats (:150-172), petapm's CIC deposit and readout (pm_iterate_one,
 * petapm.cpp:1132-1183) and the power sums of measure_power_spectrum / powerspectrum_add_mode (gravpm.cpp:323-376).
 *
 * Storage is ic_part_data's (allvars.h:8-16): double Pos, float Vel, float Disp, float Mass, and the arithmetic is what C++ makes of
 * the reference's expressions on those types:
 *   readout  Disp[k] += weight * mesh[0]               the double sum of float Disp and a double product, rounded to float - eight
 *                                                       times per component, in connection order 0..7
 *   kick     Vel[d] += (Disp[d] - Vel[d]) * hdt        Disp - Vel is a FLOAT subtraction (both operands are float), times the double
 *                                                       hdt, added to Vel in double, rounded to float
 *   drift    Pos[d] += Vel[d] * dt                     double
 *   totmass += Mass                                    double sum of float masses, in particle order, on the host
 * Positions are never wrapped: the cell is floor(Pos / CellSize) modulo Nmesh and the residual comes from the unwrapped quotient
 * (cic_setup, cic.hpp), which is what the reference's min / max region folded periodically into the pencils amounts to.
 *
 * A force, with two meshes A and B of the call's own:
 *   A  zeroed, the fixed-point CIC deposit (64-bit integer atomics: the mesh does not depend on particle order or launch shape), the
 *      unscaled r2c in place (the five-pass pipeline of fft3d.hip where it has the mesh size, hipFFT otherwise): the density spectrum
 *   -  for a force whose spectrum is saved: one read of A for BOTH power additions of the reference - measure_power_spectrum adds every
 *      mode with the CIC deconvolution weight, potential_transfer (glass.cpp:304) adds it again with weight 1 into the same sums.  That
 *      double count is the reference's behaviour, not a choice made here.  The opening force's sums are zeroed before anybody reads
 *      them (powerspectrum_zero in the next glass_force), so it skips the pass, as does a call without the spectrum pointers.
 *   B  per axis: potential_transfer and the force transfer in one pass from A (value *= pot_factor * (1.0 / k2) * f * f, f = 1, the zero
 *      mode 0; then value = i fac value, fac from a host table in the reference's expression and libm's sin), the unscaled c2r in
 *      place, and the CIC gather into float Disp.  A, the density spectrum, survives the three inverse transforms untouched, so the
 *      potential is never written out: that saves a pass over the mesh per force.
 * Between forces ONE particle kernel: second kick of step s, the two statistics sums (wave reduction, then one atomic per workgroup and
 * sum from a capped grid: one atomic per wave on the same two words cost 0.6 ms of a 0.75 ms kernel at 2 M particles), first
 * kick of step s + 1, drift.  Per particle these are the reference's operations in the reference's order, so the result is that of its
 * three loops.  The first kick + drift and the last kick + statistics are the ragged ends of the same kernel.
 * Of the context only the FFT twiddle table is touched.
 *
 * Several ranks: the same phases as entry points of their own (shq_glass_slab_*, at the end of the file) on the caller's device memory,
 * with the caller's exchanges between them (shenqi_amd/dist.py, DistGlass).  The particles stay on the owners of their CIC base planes
 * (glass_planes_kernel: cic_setup's plane, what routes a row) across the whole loop; the deposit and the gather work on a window of x
 * planes; the two power additions ride on the X forward of the y-slab and the potential + force transfer on its out-of-place X inverse
 * (fft3d.hip, fft_pass_strided MODES 7 and 8), with dense kernels for mesh sizes without a bespoke transform.  Nothing there has run on
 * more than one GPU.
 */
#include "common.hpp"
#include "mesh_common.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

namespace {

constexpr int GT = 256;

/* put_particle_to_mesh (petapm.cpp:1304-1310) with pm_iterate_one's cells and weights, accumulated in 64-bit fixed point */
__global__ __launch_bounds__(GT) void glass_deposit_kernel(long long n, const double *__restrict__ pos, const float *__restrict__ mass,
                                                          unsigned long long *mesh, int N, int zp, double cell, double scale)
{
#pragma clang fp contract(off)
    const long long p = (long long) blockIdx.x * GT + threadIdx.x;
    if(p >= n)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], cell, N, ic, res);
    const double m = (double) mass[p];
    cic_corners(ic, res, N, zp, [&](int, size_t lin, double w) {
#pragma clang fp contract(off)
        const long long q = __double2ll_rn(w * m * scale);
        atomicAdd(&mesh[lin], (unsigned long long) q);
    });
}

/* powerspectrum_add_mode (gravpm.cpp:323-356) for both of the reference's callers in one read of the density spectrum [x][y][zpc]:
 * invwindow = prod 1 / sinc^2 (measure_power_spectrum) and invwindow = 1 (potential_transfer, glass.cpp:304).
 * sums: [nbins] power, [nbins] kk, [nbins] modes (u64), norm.  Each workgroup histograms in LDS and flushes one atomic per non-empty bin. */
__global__ __launch_bounds__(GT) void glass_power_kernel(const double2 *__restrict__ spec, int N, int zpc, const double *__restrict__ sinctab,
                                                        const int32_t *__restrict__ bintab, double *sums)
{
    extern __shared__ double hist[]; /* [3][nbins] */
    const int nbins = N, Nc = N / 2 + 1;
    for(int i = threadIdx.x; i < 3 * nbins; i += GT)
        hist[i] = 0;
    __syncthreads();
    const size_t total = (size_t) N * N * Nc;
    for(size_t ip = (size_t) blockIdx.x * GT + threadIdx.x; ip < total; ip += (size_t) gridDim.x * GT) {
        const HalfMode md = half_mode(ip, N);
        const int x = md.x, y = md.y, z = md.z;
        const long long k2 = md.k2;
        const double2 v = spec[md.row * (size_t) zpc + z];
        const double m = v.x * v.x + v.y * v.y;
        if(k2 == 0) {
            sums[3 * nbins] = m; /* Norm: both callers write the same value */
            continue;
        }
        const int kint = bintab[k2];
        if(kint >= nbins)
            continue;
        const double f = sinctab[x] * sinctab[y] * sinctab[z];
        const double w = (z == 0 || z == N / 2) ? 1.0 : 2.0;
        atomicAdd(&hist[kint], w * m * f * f + w * m);
        atomicAdd(&hist[nbins + kint], 2 * (w * sqrt((double) k2)));
        atomicAdd(&hist[2 * nbins + kint], 2 * w);
    }
    __syncthreads();
    unsigned long long *nmodes = reinterpret_cast<unsigned long long *>(sums + 2 * nbins);
    for(int i = threadIdx.x; i < nbins; i += GT)
        if(hist[2 * nbins + i] != 0) {
            atomicAdd(&sums[i], hist[i]);
            atomicAdd(&sums[nbins + i], hist[nbins + i]);
            atomicAdd(&nmodes[i], (unsigned long long) hist[2 * nbins + i]);
        }
}

/* potential_transfer (glass.cpp:285-315) and force_transfer (:329-342) of one axis, from the density spectrum into the work mesh (the
 * same pitch): fac[i] = -1 * diff_kernel(kpos(i) * (2 pi / Nmesh)) * (Nmesh / BoxSize) per mesh index, made on the host */
__global__ __launch_bounds__(GT) void glass_transfer_kernel(const double2 *__restrict__ spec, double2 *__restrict__ out, int N, int zpc,
                                                           const double *__restrict__ fac, int axis, double pot_factor)
{
#pragma clang fp contract(off)
    const int Nc = N / 2 + 1;
    const size_t total = (size_t) N * N * Nc;
    const size_t ip = (size_t) blockIdx.x * GT + threadIdx.x;
    if(ip >= total)
        return;
    const HalfMode md = half_mode(ip, N);
    const int x = md.x, y = md.y, z = md.z;
    const long long k2 = md.k2;
    const size_t row = md.row;
    double2 v = spec[row * zpc + z];
    if(k2 == 0)
        v = make_double2(0.0, 0.0);
    else {
        const double f = 1.0;
        const double smth = 1.0 / k2;
        const double pf = pot_factor * smth * f * f;
        v.x *= pf;
        v.y *= pf;
    }
    const double fa = fac[axis == 0 ? x : (axis == 1 ? y : z)];
    const double tmp0 = -v.y * fa;
    const double tmp1 = v.x * fa;
    out[row * zpc + z] = make_double2(tmp0, tmp1);
}

/* pm_iterate_one with readout_force_x / y / z: the float Disp of one axis, from 0, rounded after each of the eight connections */
__global__ __launch_bounds__(GT) void glass_gather_kernel(long long n, const double *__restrict__ pos, const double *__restrict__ mesh, int N,
                                                         int zp, double cell, float *__restrict__ disp, int axis)
{
#pragma clang fp contract(off)
    const long long p = (long long) blockIdx.x * GT + threadIdx.x;
    if(p >= n)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], cell, N, ic, res);
    float acc = 0;
    cic_corners(ic, res, N, zp, [&](int, size_t lin, double w) {
#pragma clang fp contract(off)
        acc = (float) ((double) acc + w * mesh[lin]);
    });
    disp[3 * p + axis] = acc;
}

/* One step boundary of glass_evolve (glass.cpp:109-139) per particle: [second kick of the step that ends, glass_stats' two sums],
 * [first kick of the step that begins, drift].  stats (may be null without the first part): {sum Disp^2, sum Vel^2}. */
__global__ __launch_bounds__(GT) void glass_particle_kernel(long long n, double *__restrict__ pos, float *__restrict__ vel,
                                                           const float *__restrict__ disp, int ending, int beginning, double hdt, double dt,
                                                           double *stats)
{
#pragma clang fp contract(off)
    __shared__ double part[2][GT / 64];
    double disp2 = 0, vel2 = 0;
    /* a capped grid walks the particles, so that the two sums cost a few thousand atomics and not one per wave of the whole set */
    for(long long p = (long long) blockIdx.x * GT + threadIdx.x; p < n; p += (long long) gridDim.x * GT)
        for(int d = 0; d < 3; d++) {
            const float ds = disp[3 * p + d];
            float v = vel[3 * p + d];
            if(ending) {
                const float dv = ds - v; /* mind the damping term */
                v = (float) ((double) v + (double) dv * hdt);
                const double dis = ds, vv = v;
                disp2 += dis * dis;
                vel2 += vv * vv;
            }
            if(beginning) {
                const float dv = ds - v;
                v = (float) ((double) v + (double) dv * hdt);
                pos[3 * p + d] += (double) v * dt;
            }
            vel[3 * p + d] = v;
        }
    if(ending) {
        for(int off = 32; off > 0; off >>= 1) {
            disp2 += __shfl_xor(disp2, off);
            vel2 += __shfl_xor(vel2, off);
        }
        if((threadIdx.x & 63) == 0) {
            part[0][threadIdx.x >> 6] = disp2;
            part[1][threadIdx.x >> 6] = vel2;
        }
        __syncthreads();
        if(threadIdx.x < 2) {
            double t = 0;
            for(int w = 0; w < GT / 64; w++)
                t += part[threadIdx.x][w];
            atomicAdd(&stats[threadIdx.x], t);
        }
    }
}

/* super lanzcos differencing, glass.cpp:319-327 */
double diff_kernel(double w) { return 1 / 6.0 * (8 * sin(w) - sin(2 * w)); }

/* _prepare's and the transfers' tables per mesh index: fac[i] = -1 * diff_kernel(kpos(i) * (2 pi / Nmesh)) * (Nmesh / BoxSize)
 * (force_transfer, glass.cpp:337) and 1 / sinc_unnormed(kpos(i) pi / Nmesh)^2 (measure_power_spectrum, gravpm.cpp:370-374) */
void glass_index_tables(int N, double L, double *fac, double *sinc)
{
#pragma clang fp contract(off)
    for(int i = 0; i < N; i++) {
        const int k = i <= N / 2 ? i : i - N;
        fac[i] = -1 * diff_kernel(k * (2 * M_PI / N)) * (N / L);
        double tmp = (k * M_PI) / N;
        if(tmp < 1e-5 && tmp > -1e-5) {
            const double x2 = tmp * tmp;
            tmp = 1.0 - x2 / 6. + x2 * x2 / 120.;
        } else
            tmp = sin(tmp) / tmp;
        sinc[i] = 1. / (tmp * tmp);
    }
}

/* the bin of every k2 with the reference's expression (gravpm.cpp:338-339), size = Nmesh (glass.cpp:85) */
void glass_bin_table(int N, std::vector<int32_t> &bintab)
{
    const int nbins = N;
    const long long k2max = 3ll * (N / 2) * (N / 2);
    bintab.assign((size_t) k2max + 1, 0);
    const double binsperunit = (nbins - 1) / log(sqrt(3) * N / 2.0);
    for(long long k2 = 1; k2 <= k2max; k2++)
        bintab[k2] = (int32_t) floor(binsperunit * log((double) k2) / 2.);
}

/* setup_glass's loop (glass.cpp:56-66) over the sub-block x in [x0, x0 + nx), y in [y0, y0 + ny), every z, in the index order of
 * idgen_create_pos_from_index (zeldovich.cpp:77-87), from one serial mt19937(seed).
 * boost's uniform_real_distribution<double>(0, 1) on mt19937, read as one 32-bit output per draw: raw / 2^32, redrawn unless < 1.
 * That reading is not checked against a boost build (none is at hand); std::mt19937 is the same engine (its 10000th output is the
 * standard's 4123659995). */
void glass_setup_block(int Ngrid, double BoxSize, double shift, int seed, int x0, int nx, int y0, int ny, double *pos)
{
#pragma clang fp contract(off)
    std::mt19937 rng((uint32_t) seed);
    const long long n = (long long) nx * ny * Ngrid;
    for(long long i = 0; i < n; i++) {
        const long long x = i / ((long long) Ngrid * ny) + x0, y = (i % ((long long) ny * Ngrid)) / Ngrid + y0, z = i % Ngrid;
        const long long g[3] = {x, y, z};
        for(int k = 0; k < 3; k++) {
            double u;
            do
                u = (double) (uint32_t) rng() / 4294967296.0;
            while(!(u < 1));
            double P = g[k] * BoxSize / Ngrid; /* idgen_create_pos_from_index, zeldovich.cpp:77-87 */
            const double rand = BoxSize / Ngrid * 3 * (u - 0.5);
            P += shift + rand;
            pos[3 * i + k] = P;
        }
    }
}

} // namespace

/* ---- C-ABI ------------------------------------------------------------------------------ */

extern "C" int shq_glass_setup_positions(int Ngrid, double BoxSize, double shift, int seed, double *pos)
{
#pragma clang fp contract(off)
    SHQ_CHECK(pos && Ngrid >= 1 && Ngrid <= 1290, SHQ_ERR_INVALID, "glass_setup_positions: Ngrid %d outside [1, 1290] (Ngrid^3 < 2^31)", Ngrid);
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0 && isfinite(shift), SHQ_ERR_INVALID, "glass_setup_positions: BoxSize must be finite and > 0, shift finite");
    glass_setup_block(Ngrid, BoxSize, shift, seed, 0, Ngrid, 0, Ngrid, pos);
    return SHQ_OK;
}

extern "C" int shq_glass_setup_positions_block(int Ngrid, double BoxSize, double shift, int seed, const int offset[2], const int size[2], double *pos)
{
    SHQ_CHECK(pos && offset && size && Ngrid >= 1 && Ngrid <= 1290, SHQ_ERR_INVALID,
              "glass_setup_positions_block: null argument, or Ngrid %d outside [1, 1290] (Ngrid^3 < 2^31)", Ngrid);
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0 && isfinite(shift), SHQ_ERR_INVALID,
              "glass_setup_positions_block: BoxSize must be finite and > 0, shift finite");
    for(int k = 0; k < 2; k++)
        SHQ_CHECK(offset[k] >= 0 && size[k] >= 0 && offset[k] <= Ngrid - size[k], SHQ_ERR_INVALID,
                  "glass_setup_positions_block: the sub-block [%d, %d + %d) along axis %d leaves the lattice", offset[k], offset[k], size[k], k);
    glass_setup_block(Ngrid, BoxSize, shift, seed, offset[0], size[0], offset[1], size[1], pos);
    return SHQ_OK;
}

extern "C" int shq_glass_finish_power(int size, double BoxSize_in_MPC, double *kk, double *power, int64_t *nmodes, double norm, int *nonzero)
{
#pragma clang fp contract(off)
    SHQ_CHECK(kk && power && nmodes && nonzero && size >= 1, SHQ_ERR_INVALID, "glass_finish_power: null argument or size < 1");
    SHQ_CHECK(isfinite(BoxSize_in_MPC) && BoxSize_in_MPC > 0, SHQ_ERR_INVALID, "glass_finish_power: BoxSize_in_MPC must be finite and > 0");
    int nk_nz = 0;
    for(int i = 0; i < size; i++) {
        if(nmodes[i] == 0)
            continue;
        power[i] /= nmodes[i];
        power[i] /= norm;
        kk[i] /= nmodes[i];
        kk[i] *= 2 * M_PI / (BoxSize_in_MPC);
        power[i] *= pow(BoxSize_in_MPC, 3.0);
        power[nk_nz] = power[i];
        kk[nk_nz] = kk[i];
        nmodes[nk_nz] = nmodes[i];
        nk_nz++;
    }
    *nonzero = nk_nz;
    return SHQ_OK;
}

extern "C" int shq_glass_phase_ms(shq_context *ctx, double ms[4])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 4; i++)
        ms[i] = ctx->glass_ms[i];
    return SHQ_OK;
}

extern "C" int shq_glass_evolve(shq_context *ctx, const shq_glass_params *p, int64_t n, double *pos, float *vel, float *disp, const float *mass,
                                shq_glass_step *steps, double *kk, double *power, int64_t *nmodes, double *norm)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && p && pos && vel && disp && mass, SHQ_ERR_INVALID, "glass: null argument");
    /* ---- every check before anything is written */
    const int N = p->Nmesh, nsteps = p->nsteps;
    SHQ_TRY(mesh_check_size(N, "glass"));
    SHQ_CHECK(nsteps >= 0, SHQ_ERR_INVALID, "glass: nsteps %d < 0", nsteps);
    const double L = p->BoxSize;
    SHQ_CHECK(isfinite(L) && L > 0, SHQ_ERR_INVALID, "glass: BoxSize must be finite and > 0");
    SHQ_CHECK(n >= 1 && n < (1ll << 32), SHQ_ERR_INVALID, "glass: %lld particles on one rank (1 .. 2^32 - 1)", (long long) n);
    const int nspec = (kk != nullptr) + (power != nullptr) + (nmodes != nullptr) + (norm != nullptr);
    SHQ_CHECK(nspec == 0 || nspec == 4, SHQ_ERR_INVALID, "glass: kk, power, nmodes and norm come together or not at all");
    const double cellsize = L / N; /* CellSize */
    double totmass = 0;
    for(int64_t i = 0; i < n; i++) {
        SHQ_CHECK(isfinite(mass[i]), SHQ_ERR_INVALID, "glass: non-finite mass of particle %lld", (long long) i);
        totmass += mass[i];
    }
    SHQ_CHECK(isfinite(totmass) && totmass > 0, SHQ_ERR_INVALID, "glass: the total mass must be > 0 (got %g)", totmass);
    for(int64_t i = 0; i < 3 * n; i++) {
        /* beyond 2^30 cells the cell index no longer fits the readout's int */
        SHQ_CHECK(isfinite(pos[i]) && fabs(pos[i] / cellsize) < 1073741824.0, SHQ_ERR_INVALID,
                  "glass: position of particle %lld is not finite or beyond 2^30 cells: %g", (long long) (i / 3), pos[i]);
        SHQ_CHECK(isfinite(vel[i]), SHQ_ERR_INVALID, "glass: non-finite velocity of particle %lld", (long long) (i / 3));
    }
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(shq_join_pm(ctx)); /* the bespoke transforms share the context's twiddle table with a prestarted PM */
    for(int i = 0; i < 4; i++)
        ctx->glass_ms[i] = 0;

    /* _prepare, glass.cpp:233, 257 */
    double pot_factor = -1 * (-1) * pow(2 * M_PI / L, -2);
    pot_factor /= totmass;
    std::vector<double> fac((size_t) N), sinc((size_t) N);
    glass_index_tables(N, L, fac.data(), sinc.data());
    /* the deposit's fixed-point scale 2^e: the whole mass in one cell stays below 2^61 */
    int ex = 0;
    (void) frexp(totmass, &ex);
    const double scale = ldexp(1.0, 61 - ex), inv_scale = ldexp(1.0, ex - 61);

    hipStream_t s = ctx->stream;
    CallScope sc(ctx, "glass");
    SHQ_TRY(sc.mark(s));
    Fft3dRoute route = fft3d_route(N);
    const int zp = route.zp;
    const size_t padded = route.padded;
    const int nbins = N;
    const size_t nsums = 3 * (size_t) nbins + 1;
    const bool spectra = nspec == 4 && nsteps > 0;
    double *d_A, *d_B, *d_pos, *d_fac, *d_sinc, *d_stats, *d_sums = nullptr;
    float *d_vel, *d_disp, *d_mass;
    int32_t *d_bintab = nullptr;
    SHQ_TRY(sc.alloc(&d_A, padded));
    SHQ_TRY(sc.alloc(&d_B, padded));
    SHQ_TRY(sc.alloc(&d_pos, (size_t) 3 * n));
    SHQ_TRY(sc.alloc(&d_vel, (size_t) 3 * n));
    SHQ_TRY(sc.alloc(&d_disp, (size_t) 3 * n));
    SHQ_TRY(sc.alloc(&d_mass, (size_t) n));
    SHQ_TRY(sc.alloc(&d_fac, (size_t) N));
    SHQ_TRY(sc.alloc(&d_sinc, (size_t) N));
    SHQ_TRY(sc.alloc(&d_stats, (size_t) 2 * std::max(nsteps, 1)));
    std::vector<int32_t> bintab;
    if(spectra) {
        glass_bin_table(N, bintab);
        SHQ_TRY(sc.alloc(&d_bintab, bintab.size()));
        SHQ_TRY(sc.alloc(&d_sums, nsums * nsteps));
        SHQ_HIP(hipMemcpyAsync(d_bintab, bintab.data(), sizeof(int32_t) * bintab.size(), hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemsetAsync(d_sums, 0, sizeof(double) * nsums * nsteps, s));
    }
    SHQ_HIP(hipMemcpyAsync(d_pos, pos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_vel, vel, sizeof(float) * 3 * n, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_mass, mass, sizeof(float) * n, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_fac, fac.data(), sizeof(double) * N, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_sinc, sinc.data(), sizeof(double) * N, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemsetAsync(d_stats, 0, sizeof(double) * 2 * std::max(nsteps, 1), s));
    SHQ_HIP(hipMemsetAsync(d_B, 0, sizeof(double) * padded, s)); /* the pitch's padding is never written again */
    SHQ_TRY(route_plans(sc, route, true, true));
    SHQ_TRY(sc.mark(s)); /* ev[1]: uploaded */

    const size_t modes = (size_t) N * N * (N / 2 + 1);
    const size_t lds = sizeof(double) * 3 * nbins; /* <= 48 KiB at Nmesh 2048 */
    const dim3 gp(nblk(n, GT)), gm(nblk((long long) modes, GT)), gk(std::min(nblk(n, GT), 2048u));
    /* glass_force (glass.cpp:184-216); sums: where this force's power sums go, or null */
    auto force = [&](double *sums) -> int {
        SHQ_HIP(hipMemsetAsync(d_A, 0, sizeof(double) * padded, s));
        glass_deposit_kernel<<<gp, dim3(GT), 0, s>>>(n, d_pos, d_mass, reinterpret_cast<unsigned long long *>(d_A), N, zp, cellsize, scale);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(route_forward(ctx, sc, route, d_A, true, inv_scale));
        if(sums) {
            glass_power_kernel<<<dim3((unsigned) std::min<size_t>(1024, nblk((long long) modes, GT))), dim3(GT), lds, s>>>(
                reinterpret_cast<const double2 *>(d_A), N, zp / 2, d_sinc, d_bintab, sums);
            SHQ_HIP(hipGetLastError());
        }
        for(int axis = 0; axis < 3; axis++) {
            glass_transfer_kernel<<<gm, dim3(GT), 0, s>>>(reinterpret_cast<const double2 *>(d_A), reinterpret_cast<double2 *>(d_B), N, zp / 2,
                                                         d_fac, axis, pot_factor);
            SHQ_HIP(hipGetLastError());
            SHQ_TRY(route_inverse(ctx, sc, route, d_B));
            glass_gather_kernel<<<gp, dim3(GT), 0, s>>>(n, d_pos, d_B, N, zp, cellsize, d_disp, axis);
            SHQ_HIP(hipGetLastError());
        }
        return SHQ_OK;
    };

    /* ---- glass_evolve (glass.cpp:76-147).  Events: [2 + 2 i] after force i, [3 + 2 i] after the particle kernel behind it */
    const double dt = M_PI / 2, hdt = 0.5 * dt;
    SHQ_TRY(force(nullptr));
    SHQ_TRY(sc.mark(s));
    for(int step = 0; step < nsteps; step++) {
        /* the second kick and statistics of step - 1, the first kick and drift of this step */
        glass_particle_kernel<<<gk, dim3(GT), 0, s>>>(n, d_pos, d_vel, d_disp, step > 0, 1, hdt, dt, step > 0 ? d_stats + 2 * (step - 1) : nullptr);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(sc.mark(s));
        SHQ_TRY(force(spectra ? d_sums + nsums * step : nullptr));
        SHQ_TRY(sc.mark(s));
    }
    if(nsteps > 0) {
        glass_particle_kernel<<<gk, dim3(GT), 0, s>>>(n, d_pos, d_vel, d_disp, 1, 0, hdt, dt, d_stats + 2 * (nsteps - 1));
        SHQ_HIP(hipGetLastError());
    }
    SHQ_TRY(sc.mark(s));
    const size_t ev_done = sc.ev.size() - 1;

    /* ---- the one download.  Staged, so that a failure leaves the caller's arrays as they were */
    std::vector<double> h_stats((size_t) 2 * std::max(nsteps, 1)), h_sums(spectra ? nsums * nsteps : 0);
    SHQ_HIP(hipMemcpyAsync(h_stats.data(), d_stats, sizeof(double) * h_stats.size(), hipMemcpyDeviceToHost, s));
    if(spectra)
        SHQ_HIP(hipMemcpyAsync(h_sums.data(), d_sums, sizeof(double) * h_sums.size(), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s)); /* every kernel has run without an error before the caller's arrays change */
    SHQ_HIP(hipMemcpyAsync(pos, d_pos, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipMemcpyAsync(vel, d_vel, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipMemcpyAsync(disp, d_disp, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, s));
    SHQ_TRY(sc.mark(s));
    SHQ_HIP(hipStreamSynchronize(s));

    double t_x = 0, t_v = 0, t_f = 0;
    for(int step = 0; step < nsteps; step++) {
        t_x += hdt;
        t_v += dt;
        t_f = t_x;
        t_x += hdt;
        if(steps) {
            steps[step].t_f = t_f;
            steps[step].t_v = t_v;
            steps[step].t_x = t_x;
            steps[step].force_std = sqrt(h_stats[2 * step] / (double) n);
            steps[step].vel_std = sqrt(h_stats[2 * step + 1] / (double) n);
        }
        if(spectra) {
            const double *src = h_sums.data() + nsums * step;
            memcpy(power + (size_t) nbins * step, src, sizeof(double) * nbins);
            memcpy(kk + (size_t) nbins * step, src + nbins, sizeof(double) * nbins);
            memcpy(nmodes + (size_t) nbins * step, src + 2 * nbins, sizeof(int64_t) * nbins);
            norm[step] = src[3 * nbins];
        }
    }
    ctx->glass_ms[0] = sc.ms(0, 1);
    for(size_t i = 1; i < ev_done; i++)
        ctx->glass_ms[(i % 2) ? 1 : 2] += sc.ms(i, i + 1); /* odd -> even: a force; even -> odd: a particle kernel */
    ctx->glass_ms[3] = sc.ms(0, sc.ev.size() - 1);
    return SHQ_OK;
}

/* ---- the same phases on a rank's slab (several ranks: shenqi_amd/dist.py, DistGlass) --------------------------------------------
 * Every pointer named d_ is device memory of the caller (torch tensors).  The density's deposit and a force's real mesh live on the
 * rank's window of x planes [nalloc][N][zp] (zp = shq_glass_slab_pitch, or N + 2 without a bespoke transform), the spectrum on a y-slab
 * [N][nyl][zp / 2] complex.  None of these calls reads or writes the PM's state, the one-rank resident Zel'dovich field or the
 * Zel'dovich slab family's tables: the twiddles, the tables, the flag and the sums are the context's gls_ ones. */
namespace {

/* the CIC base plane of every particle, with the cell arithmetic the deposit and the gather use (cic_setup): what routes a particle */
__global__ __launch_bounds__(GT) void glass_planes_kernel(long long n, const double *__restrict__ pos, int N, double cell, int32_t *__restrict__ planes)
{
    const long long p = (long long) blockIdx.x * GT + threadIdx.x;
    if(p >= n)
        return;
    int ic;
    double res;
    cic_setup(pos[3 * p], cell, N, ic, res);
    planes[p] = ic;
}

/* glass_deposit_kernel on a rank's window [nalloc][N][zp] whose plane 0 is the mesh plane plane0: the own planes and one ghost plane
 * behind them (nplanes = N: the periodic mesh).  A particle whose base plane is not an own plane raises *oob and deposits nothing. */
__global__ __launch_bounds__(GT) void glass_slab_deposit_kernel(long long n, const double *__restrict__ pos, const float *__restrict__ mass,
                                                               unsigned long long *mesh, int N, int zp, double cell, double scale, int plane0,
                                                               int nplanes, int nalloc, int *oob)
{
#pragma clang fp contract(off)
    const long long p = (long long) blockIdx.x * GT + threadIdx.x;
    if(p >= n)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], cell, N, ic, res);
    if(xloc(ic[0], plane0, N) >= nplanes) {
        *oob = 1;
        return;
    }
    const double m = (double) mass[p];
    cic_corners<true>(
        ic, res, N, zp,
        [&](int, size_t lin, double w) {
#pragma clang fp contract(off)
            const long long q = __double2ll_rn(w * m * scale);
            atomicAdd(&mesh[lin], (unsigned long long) q);
        },
        plane0, nalloc, oob);
}

/* glass_gather_kernel on such a window: the own planes and the right-hand neighbour's first plane behind them */
__global__ __launch_bounds__(GT) void glass_slab_gather_kernel(long long n, const double *__restrict__ pos, const double *__restrict__ mesh, int N,
                                                              int zp, double cell, int plane0, int nplanes, int nalloc, float *__restrict__ disp,
                                                              int axis, int *oob)
{
#pragma clang fp contract(off)
    const long long p = (long long) blockIdx.x * GT + threadIdx.x;
    if(p >= n)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], cell, N, ic, res);
    if(xloc(ic[0], plane0, N) >= nplanes) {
        *oob = 1;
        return;
    }
    float acc = 0;
    int outside = 0;
    cic_corners<true>(
        ic, res, N, zp,
        [&](int, size_t lin, double w) {
#pragma clang fp contract(off)
            acc = (float) ((double) acc + w * mesh[lin]);
        },
        plane0, nalloc, &outside);
    if(outside)
        *oob = 1;
    else
        disp[3 * p + axis] = acc;
}

/* glass_power_kernel on a rank's dense y-slab [x][row][N / 2 + 1], row = mesh row y0 + row: the same operations per mode */
__global__ __launch_bounds__(GT) void glass_slab_power_kernel(const double2 *__restrict__ spec, int N, int y0, int nyl, const double *__restrict__ sinctab,
                                                             const int32_t *__restrict__ bintab, double *sums)
{
    extern __shared__ double hist[]; /* [3][nbins] */
    const int nbins = N, Nc = N / 2 + 1;
    for(int i = threadIdx.x; i < 3 * nbins; i += GT)
        hist[i] = 0;
    __syncthreads();
    const size_t total = (size_t) N * nyl * Nc;
    for(size_t ip = (size_t) blockIdx.x * GT + threadIdx.x; ip < total; ip += (size_t) gridDim.x * GT) {
        const int z = (int) (ip % Nc), row = (int) ((ip / Nc) % nyl), x = (int) (ip / ((size_t) Nc * nyl));
        const int y = y0 + row;
        const int kx = x <= N / 2 ? x : x - N, ky = y <= N / 2 ? y : y - N;
        const long long k2 = (long long) kx * kx + (long long) ky * ky + (long long) z * z;
        const double2 v = spec[ip];
        const double m = v.x * v.x + v.y * v.y;
        if(k2 == 0) {
            sums[3 * nbins] = m;
            continue;
        }
        const int kint = bintab[k2];
        if(kint >= nbins)
            continue;
        const double f = sinctab[x] * sinctab[y] * sinctab[z];
        const double w = (z == 0 || z == N / 2) ? 1.0 : 2.0;
        atomicAdd(&hist[kint], w * m * f * f + w * m);
        atomicAdd(&hist[nbins + kint], 2 * (w * sqrt((double) k2)));
        atomicAdd(&hist[2 * nbins + kint], 2 * w);
    }
    __syncthreads();
    unsigned long long *nmodes = reinterpret_cast<unsigned long long *>(sums + 2 * nbins);
    for(int i = threadIdx.x; i < nbins; i += GT)
        if(hist[2 * nbins + i] != 0) {
            atomicAdd(&sums[i], hist[i]);
            atomicAdd(&sums[nbins + i], hist[nbins + i]);
            atomicAdd(&nmodes[i], (unsigned long long) hist[2 * nbins + i]);
        }
}

/* glass_transfer_kernel on such a slab (out may be spec) */
__global__ __launch_bounds__(GT) void glass_slab_transfer_kernel(const double2 *spec, double2 *out, int N, int y0, int nyl,
                                                                const double *__restrict__ fac, int axis, double pot_factor)
{
#pragma clang fp contract(off)
    const int Nc = N / 2 + 1;
    const size_t total = (size_t) N * nyl * Nc;
    const size_t ip = (size_t) blockIdx.x * GT + threadIdx.x;
    if(ip >= total)
        return;
    const int z = (int) (ip % Nc), row = (int) ((ip / Nc) % nyl), x = (int) (ip / ((size_t) Nc * nyl));
    const int y = y0 + row;
    const int kx = x <= N / 2 ? x : x - N, ky = y <= N / 2 ? y : y - N;
    const long long k2 = (long long) kx * kx + (long long) ky * ky + (long long) z * z;
    double2 v = spec[ip];
    if(k2 == 0)
        v = make_double2(0.0, 0.0);
    else {
        const double f = 1.0;
        const double smth = 1.0 / k2;
        const double pf = pot_factor * smth * f * f;
        v.x *= pf;
        v.y *= pf;
    }
    const double fa = fac[axis == 0 ? x : (axis == 1 ? y : z)];
    const double tmp0 = -v.y * fa;
    const double tmp1 = v.x * fa;
    out[ip] = make_double2(tmp0, tmp1);
}

} // namespace

extern "C" int shq_glass_slab_pitch(int Nmesh) { return slab_pitch(Nmesh); }

extern "C" int shq_glass_slab_tables(shq_context *ctx, int Nmesh, double BoxSize, double totmass)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "glass_slab_tables: null context");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "glass_slab_tables"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0, SHQ_ERR_INVALID, "glass_slab_tables: BoxSize must be finite and > 0");
    SHQ_CHECK(isfinite(totmass) && totmass > 0, SHQ_ERR_INVALID, "glass_slab_tables: the total mass must be > 0 (got %g)", totmass);
    SHQ_HIP(hipSetDevice(ctx->device));
    double pot_factor = -1 * (-1) * pow(2 * M_PI / BoxSize, -2); /* _prepare, glass.cpp:233, 257 */
    pot_factor /= totmass;
    if(ctx->gls_tabs_n != N || ctx->gls_box != BoxSize) {
        std::vector<double> tabs(2 * (size_t) N);
        glass_index_tables(N, BoxSize, tabs.data(), tabs.data() + N);
        std::vector<int32_t> bintab;
        glass_bin_table(N, bintab);
        ctx->gls_tabs_n = 0;
        SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* a pass may still read the previous tables */
        SHQ_TRY(ctx->gls_tabs.reserve(tabs.size()));
        SHQ_TRY(ctx->gls_bin.reserve(bintab.size()));
        SHQ_HIP(hipMemcpy(ctx->gls_tabs.ptr, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice));
        SHQ_HIP(hipMemcpy(ctx->gls_bin.ptr, bintab.data(), sizeof(int32_t) * bintab.size(), hipMemcpyHostToDevice));
        ctx->gls_tabs_n = N;
        ctx->gls_box = BoxSize;
    }
    ctx->gls_totmass = totmass;
    ctx->gls_pot_factor = pot_factor;
    return SHQ_OK;
}

extern "C" int shq_glass_slab_planes(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, int64_t n, void *d_planes)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "glass_slab_planes: null context");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_pos && d_planes)), SHQ_ERR_INVALID, "glass_slab_planes: bad particle arrays");
    SHQ_TRY(mesh_check_size(Nmesh, "glass_slab_planes"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0, SHQ_ERR_INVALID, "glass_slab_planes: BoxSize must be finite and > 0");
    SHQ_HIP(hipSetDevice(ctx->device));
    if(n > 0)
        glass_planes_kernel<<<dim3(nblk(n, GT)), dim3(GT), 0, ctx->stream>>>(n, (const double *) d_pos, Nmesh, BoxSize / Nmesh, (int32_t *) d_planes);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

extern "C" int shq_glass_slab_deposit(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, const void *d_mass, int64_t n, int exp, int plane0,
                                      int nplanes, int nalloc, void *d_mesh)
{
    SHQ_CHECK(ctx && d_mesh, SHQ_ERR_INVALID, "glass_slab_deposit: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_pos && d_mass)), SHQ_ERR_INVALID, "glass_slab_deposit: bad particle arrays");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "glass_slab_deposit"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0, SHQ_ERR_INVALID, "glass_slab_deposit: BoxSize must be finite and > 0");
    SHQ_CHECK(slab_window_ok(N, plane0, nplanes, nalloc), SHQ_ERR_INVALID, "glass_slab_deposit: bad slab geometry");
    SHQ_CHECK(exp > -900 && exp < 900, SHQ_ERR_INVALID, "glass_slab_deposit: bad scale exponent %d", exp);
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int zp = fft3d_route(N).zp;
    SHQ_TRY(slab_flag_reset(ctx, ctx->gls_flag));
    SHQ_HIP(hipMemsetAsync(d_mesh, 0, sizeof(double) * (size_t) nalloc * N * zp, s));
    if(n > 0)
        glass_slab_deposit_kernel<<<dim3(nblk(n, GT)), dim3(GT), 0, s>>>(n, (const double *) d_pos, (const float *) d_mass,
                                                                          (unsigned long long *) d_mesh, N, zp, BoxSize / N, ldexp(1.0, 61 - exp),
                                                                          plane0, nplanes, nalloc, ctx->gls_flag.ptr);
    SHQ_HIP(hipGetLastError());
    int oob;
    SHQ_TRY(slab_flag_read(ctx, ctx->gls_flag.ptr, &oob));
    SHQ_CHECK(!oob, SHQ_ERR_INVALID, "glass_slab_deposit: a particle lies outside this rank's slab (planes %d .. %d)", plane0, plane0 + nplanes - 1);
    return SHQ_OK;
}

extern "C" int shq_glass_slab_fft_yz(shq_context *ctx, int Nmesh, void *d_planes, int nplanes, int direction, int exp, void *d_packed, int nranks)
{
    return slab_fft_yz(ctx, "glass_slab_fft_yz", &shq_context::gls_tw, &shq_context::gls_tw_n, Nmesh, d_planes, nplanes, direction, exp, d_packed, nranks);
}

extern "C" int shq_glass_slab_xforward(shq_context *ctx, int Nmesh, void *d_spec, int y0, int nyl, void *d_sums)
{
    SHQ_CHECK(ctx && d_spec, SHQ_ERR_INVALID, "glass_slab_xforward: null argument");
    const int N = Nmesh, zp = shq_glass_slab_pitch(N);
    SHQ_CHECK(zp > 0, SHQ_ERR_INVALID, "glass_slab_xforward: mesh size %d has no bespoke FFT", N);
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N, SHQ_ERR_INVALID, "glass_slab_xforward: bad slab geometry");
    SHQ_CHECK(!d_sums || ctx->gls_tabs_n == N, SHQ_ERR_STATE, "glass_slab_xforward: no tables of mesh size %d (shq_glass_slab_tables first)", N);
    SHQ_HIP(hipSetDevice(ctx->device));
    shq_fft_opts o;
    SHQ_TRY(slab_twiddles(ctx, ctx->gls_tw, ctx->gls_tw_n, N, &o.tw));
    o.nslab = nyl;
    o.y0 = y0;
    if(d_sums) {
        o.ps = (double *) d_sums;
        o.bintab = ctx->gls_bin.ptr;
    }
    return shq_fft3d_run(ctx, (double *) d_spec, N, zp, SHQ_FFT_X_GLASS_FORWARD, false, 1.0, d_sums ? ctx->gls_tabs.ptr + N : nullptr, 0, 0, o);
}

extern "C" int shq_glass_slab_xtransfer(shq_context *ctx, int Nmesh, const void *d_spec, void *d_out, int y0, int nyl, int axis)
{
    SHQ_CHECK(ctx && d_spec && d_out && d_spec != d_out, SHQ_ERR_INVALID, "glass_slab_xtransfer: null argument, or the pass asked to run in place");
    const int N = Nmesh, zp = shq_glass_slab_pitch(N);
    SHQ_CHECK(zp > 0, SHQ_ERR_INVALID, "glass_slab_xtransfer: mesh size %d has no bespoke FFT", N);
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N && axis >= 0 && axis <= 2, SHQ_ERR_INVALID, "glass_slab_xtransfer: bad slab geometry or axis");
    SHQ_CHECK(ctx->gls_tabs_n == N, SHQ_ERR_STATE, "glass_slab_xtransfer: no tables of mesh size %d (shq_glass_slab_tables first)", N);
    SHQ_HIP(hipSetDevice(ctx->device));
    shq_fft_opts o;
    SHQ_TRY(slab_twiddles(ctx, ctx->gls_tw, ctx->gls_tw_n, N, &o.tw));
    o.nslab = nyl;
    o.y0 = y0;
    o.modefac = ctx->gls_tabs.ptr; /* fac[N] */
    o.zel_axis = axis;
    o.out = (double *) d_out;
    return shq_fft3d_run(ctx, (double *) const_cast<void *>(d_spec), N, zp, SHQ_FFT_X_GLASS, false, 1.0, nullptr, 0, ctx->gls_pot_factor, o);
}

extern "C" int shq_glass_slab_power(shq_context *ctx, int Nmesh, const void *d_spec, int y0, int nyl, void *d_sums)
{
    SHQ_CHECK(ctx && d_spec && d_sums, SHQ_ERR_INVALID, "glass_slab_power: null argument");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "glass_slab_power"));
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N, SHQ_ERR_INVALID, "glass_slab_power: bad slab geometry");
    SHQ_CHECK(ctx->gls_tabs_n == N, SHQ_ERR_STATE, "glass_slab_power: no tables of mesh size %d (shq_glass_slab_tables first)", N);
    SHQ_HIP(hipSetDevice(ctx->device));
    const long long modes = (long long) N * nyl * (N / 2 + 1);
    glass_slab_power_kernel<<<dim3((unsigned) std::min<size_t>(1024, nblk(modes, GT))), dim3(GT), sizeof(double) * 3 * N, ctx->stream>>>(
        (const double2 *) d_spec, N, y0, nyl, ctx->gls_tabs.ptr + N, ctx->gls_bin.ptr, (double *) d_sums);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

extern "C" int shq_glass_slab_transfer(shq_context *ctx, int Nmesh, const void *d_spec, void *d_out, int y0, int nyl, int axis)
{
    SHQ_CHECK(ctx && d_spec && d_out, SHQ_ERR_INVALID, "glass_slab_transfer: null argument");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "glass_slab_transfer"));
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N && axis >= 0 && axis <= 2, SHQ_ERR_INVALID, "glass_slab_transfer: bad slab geometry or axis");
    SHQ_CHECK(ctx->gls_tabs_n == N, SHQ_ERR_STATE, "glass_slab_transfer: no tables of mesh size %d (shq_glass_slab_tables first)", N);
    SHQ_HIP(hipSetDevice(ctx->device));
    const long long modes = (long long) N * nyl * (N / 2 + 1);
    glass_slab_transfer_kernel<<<dim3(nblk(modes, GT)), dim3(GT), 0, ctx->stream>>>((const double2 *) d_spec, (double2 *) d_out, N, y0, nyl,
                                                                                  ctx->gls_tabs.ptr, axis, ctx->gls_pot_factor);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

extern "C" int shq_glass_slab_gather(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, int64_t n, const void *d_mesh, int plane0,
                                     int nplanes, int nalloc, void *d_disp, int axis)
{
    SHQ_CHECK(ctx && d_mesh, SHQ_ERR_INVALID, "glass_slab_gather: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_pos && d_disp)), SHQ_ERR_INVALID, "glass_slab_gather: bad particle arrays");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "glass_slab_gather"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0 && axis >= 0 && axis <= 2, SHQ_ERR_INVALID, "glass_slab_gather: BoxSize must be finite and > 0, axis 0 .. 2");
    SHQ_CHECK(slab_window_ok(N, plane0, nplanes, nalloc), SHQ_ERR_INVALID, "glass_slab_gather: bad slab geometry");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHQ_TRY(slab_flag_reset(ctx, ctx->gls_flag));
    if(n > 0)
        glass_slab_gather_kernel<<<dim3(nblk(n, GT)), dim3(GT), 0, s>>>(n, (const double *) d_pos, (const double *) d_mesh, N, fft3d_route(N).zp,
                                                                         BoxSize / N, plane0, nplanes, nalloc, (float *) d_disp, axis, ctx->gls_flag.ptr);
    SHQ_HIP(hipGetLastError());
    int oob;
    SHQ_TRY(slab_flag_read(ctx, ctx->gls_flag.ptr, &oob));
    SHQ_CHECK(!oob, SHQ_ERR_INVALID, "glass_slab_gather: a particle lies outside this rank's slab (planes %d .. %d)", plane0, plane0 + nplanes - 1);
    return SHQ_OK;
}

extern "C" int shq_glass_slab_particles(shq_context *ctx, int64_t n, void *d_pos, void *d_vel, const void *d_disp, int ending, int beginning, double sums[2])
{
    SHQ_CHECK(ctx && sums, SHQ_ERR_INVALID, "glass_slab_particles: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_pos && d_vel && d_disp)), SHQ_ERR_INVALID, "glass_slab_particles: bad particle arrays");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHQ_TRY(ctx->gls_stats.reserve(2));
    SHQ_HIP(hipMemsetAsync(ctx->gls_stats.ptr, 0, sizeof(double) * 2, s));
    const double dt = M_PI / 2, hdt = 0.5 * dt; /* glass_evolve, glass.cpp:98-99 */
    if(n > 0)
        glass_particle_kernel<<<dim3(std::min(nblk(n, GT), 2048u)), dim3(GT), 0, s>>>(n, (double *) d_pos, (float *) d_vel, (const float *) d_disp,
                                                                                      ending != 0, beginning != 0, hdt, dt, ctx->gls_stats.ptr);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(sums, ctx->gls_stats.ptr, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    return SHQ_OK;
}
