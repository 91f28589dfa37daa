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

} // namespace

/* ---- C-ABI ------------------------------------------------------------------------------ */

extern "C" int shq_glass_setup_positions(int Ngrid, double BoxSize, double shift, int seed, double *pos)
{
#pragma clang fp contract(off)
    SHQ_CHECK(pos && Ngrid >= 1 && Ngrid <= 1290, SHQ_ERR_INVALID, "glass_setup_positions: Ngrid %d outside [1, 1290] (Ngrid^3 < 2^31)", Ngrid);
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0 && isfinite(shift), SHQ_ERR_INVALID, "glass_setup_positions: BoxSize must be finite and > 0, shift finite");
    /* boost's uniform_real_distribution<double>(0, 1) on mt19937, read as one 32-bit output per draw: raw / 2^32, redrawn unless < 1.
     * That reading is not checked against a boost build (none is at hand); std::mt19937 is the same engine (its 10000th output is the
     * standard's 4123659995). */
    std::mt19937 rng((uint32_t) seed);
    const long long n = (long long) Ngrid * Ngrid * Ngrid;
    for(long long i = 0; i < n; i++) {
        const long long x = i / ((long long) Ngrid * Ngrid), y = (i % ((long long) Ngrid * Ngrid)) / Ngrid, z = i % Ngrid;
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
    for(int i = 0; i < N; i++) {
        const int k = i <= N / 2 ? i : i - N;
        fac[i] = -1 * diff_kernel(k * (2 * M_PI / N)) * (N / L); /* force_transfer, glass.cpp:337 */
        /* measure_power_spectrum, gravpm.cpp:370-374, with sinc_unnormed */
        double tmp = (k * M_PI) / N;
        if(tmp < 1e-5 && tmp > -1e-5) {
            const double x2 = tmp * tmp;
            tmp = 1.0 - x2 / 6. + x2 * x2 / 120.;
        } else
            tmp = sin(tmp) / tmp;
        sinc[i] = 1. / (tmp * tmp);
    }
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
        /* the bin of every k2 with the reference's expression (gravpm.cpp:338-339), size = Nmesh (glass.cpp:85) */
        const long long k2max = 3ll * (N / 2) * (N / 2);
        bintab.assign((size_t) k2max + 1, 0);
        const double binsperunit = (nbins - 1) / log(sqrt(3) * N / 2.0);
        for(long long k2 = 1; k2 <= k2max; k2++)
            bintab[k2] = (int32_t) floor(binsperunit * log((double) k2) / 2.);
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
