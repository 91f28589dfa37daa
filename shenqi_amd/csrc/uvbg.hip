/* uvbg.hip — the excursion-set reionisation (EXCUR_REION) on the device for one rank: calculate_uvbg (libgadget/uvbg.cpp:474-597) with
 * petapm_reion (petapm.cpp:495-685) in one call.
 *
 *  - init_particle_uvbg (uvbg.cpp:474-507) is a particle kernel that also takes the three fields' sums for their fixed-point scales;
 *  - ONE particle pass deposits mass, stellar mass x f_esc and Sfr x f_esc in 64-bit fixed point (the PM's deposit arithmetic, pm.hip):
 *    the grids do not depend on the particle order;
 *  - each field is transformed once (the transposing pipeline's forward half, fft3d.hip part 1) and its spectrum is kept;
 *  - per radius and field the X inverse tile reads the kept spectrum, applies (v / ncell) T_R[k2] (divide_by_ncell, then filter_pm, with
 *    T_R made on the host by shq_uvbg_filter_table) and the Y / Z inverses land in the field's real mesh (part 3); then one cell kernel
 *    does reion_loop_pm (uvbg.cpp:322-459) over the three meshes;
 *  - readout_J21 (uvbg.cpp:461-472) takes the maximum J21 of a gas particle's 8 CIC cells.
 * Mesh sizes the bespoke pipeline does not have go through hipFFT plans of the call's own with a filter kernel between them.
 * The call allocates everything it uses and frees it before it returns: nothing of the context's PM state is touched.
 */
#include "mesh_common.hpp"
#include <future>
#include <math.h>
#include <string.h>

/* physconst.h */
#define UVBG_SOLAR_MASS 1.989e33
#define UVBG_PLANCK 6.6262e-27
#define UVBG_PROTONMASS 1.6726e-24
#define UVBG_SEC_PER_YEAR 3.155e7
#define UVBG_HYDROGEN_MASSFRAC 0.76
#define UVBG_FLOAT_REL_TOL ((float) 1e-5) /* uvbg.cpp:29 */
#define UVBG_MAX_R_ITERATIONS 10000       /* petapm.cpp:527 */

namespace {

/* libm through pointers the compiler cannot see through, so that no call is folded or turned into arithmetic: the tables must hold
 * what glibc's sinf / cosf / powf / pow return */
float (*volatile libm_sinf)(float) = sinf;
float (*volatile libm_cosf)(float) = cosf;
float (*volatile libm_powf)(float, float) = powf;
double (*volatile libm_pow)(double, double) = pow;

constexpr int UV_T = 256;
constexpr int UV_CELL_BLOCKS = 2048; /* fixed grid of the cell kernel: its partial sums, and so the global xHI, do not depend on the card */

/* sum of a block's values in a fixed order (thread 0 gets the total) */
__device__ __forceinline__ double block_sum(double v, double *lds)
{
    lds[threadIdx.x] = v;
    __syncthreads();
    for(int s = UV_T / 2; s > 0; s >>= 1) {
        if((int) threadIdx.x < s)
            lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

/* init_particle_uvbg (uvbg.cpp:474-507): f_esc of stars with f_esc != 0, and of gas with ReionUseParticleSFR, becomes
 * min(Norm (f_esc conv)^Scaling, 1); a negative result raises *neg.  Per block: the sums of |Mass|, |Mass f_esc| (Type 4) and
 * |Sfr f_esc| (Type 0) that pick the deposit scales. */
__global__ __launch_bounds__(UV_T) void uvbg_fesc_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                         double *fesc, const double *__restrict__ sfr, int use_sfr, double norm, double scaling,
                                                         double conv, double *part, int *neg)
{
    __shared__ double lds[UV_T];
    double s0 = 0, s1 = 0, s2 = 0;
    for(long long i = (long long) blockIdx.x * UV_T + threadIdx.x; i < n; i += (long long) gridDim.x * UV_T) {
        const int t = pflags[i] >> 4;
        double f = fesc[i];
        if(((t == 0 && use_sfr) || t == 4) && f != 0) {
            double ft = norm * pow(f * conv, scaling);
            if(ft > 1)
                ft = 1;
            if(ft < 0)
                *neg = 1;
            f = ft;
            fesc[i] = f;
        }
        const double m = posm[i].w;
        s0 += fabs(m);
        if(t == 4)
            s1 += fabs(m * f);
        if(t == 0 && use_sfr)
            s2 += fabs(sfr[i] * f);
    }
    s0 = block_sum(s0, lds);
    s1 = block_sum(s1, lds);
    s2 = block_sum(s2, lds);
    if(threadIdx.x == 0) {
        part[3 * blockIdx.x] = s0;
        part[3 * blockIdx.x + 1] = s1;
        part[3 * blockIdx.x + 2] = s2;
    }
}

/* one block: out[k] = sum over the nb partials [nb][k], k < 3, in a fixed order */
__global__ __launch_bounds__(UV_T) void uvbg_sum_kernel(const double *__restrict__ part, int nb, double *out)
{
    __shared__ double lds[UV_T];
    for(int k = 0; k < 3; k++) {
        double s = 0;
        for(int b = threadIdx.x; b < nb; b += UV_T)
            s += part[3 * b + k];
        s = block_sum(s, lds);
        if(threadIdx.x == 0)
            out[k] = s;
    }
}

/* put_particle_to_mesh / put_star_to_mesh / put_sfr_to_mesh (petapm.cpp:1304-1328) in one pass: weight * Mass [* f_esc] in fixed point */
__global__ __launch_bounds__(UV_T) void uvbg_deposit_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                            const double *__restrict__ fesc, const double *__restrict__ sfr, int use_sfr, int N,
                                                            int zp, double cell, double sc0, double sc1, double sc2, unsigned long long *m0,
                                                            unsigned long long *m1, unsigned long long *m2)
{
    const long long i = (long long) blockIdx.x * UV_T + threadIdx.x;
    if(i >= n)
        return;
    const double4 p = posm[i];
    const int t = pflags[i] >> 4;
    const bool star = t == 4, gas = t == 0 && use_sfr;
    const double f = (star || gas) ? fesc[i] : 0.0;
    const double s = gas ? sfr[i] : 0.0;
    int ic[3];
    double res[3];
    cic_cell3(p.x, p.y, p.z, cell, N, ic, res);
    cic_corners(ic, res, N, zp, [&](int, size_t lin, double w) {
        const long long q0 = __double2ll_rn(w * p.w * sc0);
        if(q0)
            atomicAdd(&m0[lin], (unsigned long long) q0);
        if(star) {
            const long long q = __double2ll_rn(w * p.w * f * sc1);
            if(q)
                atomicAdd(&m1[lin], (unsigned long long) q);
        }
        if(gas) {
            const long long q = __double2ll_rn(w * s * f * sc2);
            if(q)
                atomicAdd(&m2[lin], (unsigned long long) q);
        }
    });
}

/* hipFFT route: divide_by_ncell then filter_pm on the kept [x][y][z'] half spectrum, into the field's mesh */
__global__ void uvbg_filter_kernel(const double2 *__restrict__ spec, double2 *out, int N, const double *__restrict__ fac, int fac_mask, int ncell)
{
#pragma clang fp contract(off)
    const int Nc = N / 2 + 1;
    const size_t n = (size_t) N * N * Nc;
    const double nc = (double) ncell;
    for(size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        const double T = fac[(int) half_mode(i, N).k2 & fac_mask];
        const double2 v = spec[i];
        out[i] = make_double2((v.x / nc) * T, (v.y / nc) * T);
    }
}

/* the per-radius scalars of reion_loop_pm, formed on the host in the reference's order */
struct UvbgCell {
    double deltax_conv, rtom, R, pixel_volume, inv_eff, eff, sfr_mass_unit, sfr_time_unit, sfr_timescale, J21c;
    int use_sfr, last;
};

/* reion_loop_pm (uvbg.cpp:322-459) for every cell: clamp, f_coll_stars, sfr_density, J21_aux, the ionisation test; on the last step the
 * partial ionisations and the block's sums of xHI, xHI density_over_mean and density_over_mean */
__global__ __launch_bounds__(UV_T) void uvbg_cell_kernel(const double *__restrict__ mass, const double *__restrict__ star,
                                                         const double *__restrict__ sfr, int N, int zp, const UvbgCell c, float *J21, float *xHI,
                                                         double *part)
{
#pragma clang fp contract(off)
    __shared__ double lds[UV_T];
    const long long ncell = (long long) N * N * N;
    double s0 = 0, s1 = 0, s2 = 0;
    for(long long g = (long long) blockIdx.x * UV_T + threadIdx.x; g < ncell; g += (long long) gridDim.x * UV_T) {
        const long long row = g / N;
        const size_t m = (size_t) row * zp + (size_t) (g - row * N);
        const double mr = fmax(mass[m], 0.0), sr = fmax(star[m], 0.0);
        const double density_over_mean = mr * c.deltax_conv;
        const double f_coll_stars = sr / (c.rtom * density_over_mean) * (4.0 / 3.0) * M_PI * c.R * c.R * c.R / c.pixel_volume;
        double sfr_density;
        if(c.use_sfr)
            sfr_density = fmax(sfr[m], 0.0) / c.pixel_volume / c.sfr_mass_unit * c.sfr_time_unit;
        else
            sfr_density = sr / c.sfr_timescale / c.pixel_volume;
        const float J21_aux = (float) (sfr_density * c.J21c);
        float x = xHI[g];
        if(f_coll_stars > c.inv_eff) {
            if(x > UVBG_FLOAT_REL_TOL)
                J21[g] = J21_aux;
            x = 0.0f;
            xHI[g] = x;
        } else if(c.last && x > UVBG_FLOAT_REL_TOL) {
            x = (float) (1.0 - f_coll_stars * c.eff);
            xHI[g] = x;
        }
        if(c.last) {
            const double d = c.deltax_conv * mr;
            s0 += (double) x;
            s1 += (double) x * d;
            s2 += d;
        }
    }
    if(!c.last)
        return;
    s0 = block_sum(s0, lds);
    s1 = block_sum(s1, lds);
    s2 = block_sum(s2, lds);
    if(threadIdx.x == 0) {
        part[3 * blockIdx.x] = s0;
        part[3 * blockIdx.x + 1] = s1;
        part[3 * blockIdx.x + 2] = s2;
    }
}

__global__ void uvbg_fill_kernel(float *a, size_t n, float v)
{
    for(size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x)
        a[i] = v;
}

/* readout_J21 through pm_iterate_one (petapm.cpp:1133-1189, uvbg.cpp:461-472): every one of a gas particle's 8 CIC cells, weight 0
 * included, in connection order */
__global__ __launch_bounds__(UV_T) void uvbg_readout_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                            const float *__restrict__ J21, int N, double cell, double zre_now, double *local_J21,
                                                            double *zreion)
{
    const long long i = (long long) blockIdx.x * UV_T + threadIdx.x;
    if(i >= n || (pflags[i] >> 4) != 0)
        return;
    const double4 p = posm[i];
    int ic[3];
    double res[3];
    cic_cell3(p.x, p.y, p.z, cell, N, ic, res);
    double lj = 0.0; /* init_particle_uvbg's reset */
    double zr = zreion[i];
    cic_corners(ic, res, N, N, [&](int, size_t lin, double) { /* the grid is dense [N]^3; the weight plays no part */
        const double v = (double) J21[lin];
        if(v > lj) {
            lj = v;
            if(zr == -1)
                zr = zre_now;
        }
    });
    local_J21[i] = lj;
    zreion[i] = zr;
}

} // namespace

/* ---- C-ABI ------------------------------------------------------------------------------ */

extern "C" int shq_uvbg_filter_table(int filter_type, int Nmesh, double BoxSize, double R, double *table)
{
#pragma clang fp contract(off)
    SHQ_CHECK(table && Nmesh >= 2 && BoxSize > 0 && filter_type >= 0 && filter_type <= 2, SHQ_ERR_INVALID,
              "uvbg_filter_table: bad arguments (filter type %d, Nmesh %d)", filter_type, Nmesh);
    const long long h = Nmesh / 2, n = 3 * h * h + 1;
    for(long long k2 = 0; k2 < n; k2++) {
        /* filter_pm, uvbg.cpp:218-250: the Radius is pm->G */
        const double k_mag = sqrt((double) k2) * (2 * M_PI / Nmesh) * (Nmesh / BoxSize);
        double kR = k_mag * R;
        double f = 1.0;
        if(filter_type == 0) {
            if(kR > 1e-4) {
                const float kf = (float) kR;
                f = 3.0 * (libm_sinf(kf) / libm_powf(kf, 3) - libm_cosf(kf) / libm_powf(kf, 2));
            }
        } else if(filter_type == 1) {
            kR *= 0.413566994;
            if(kR > 1)
                f = 0.0;
        } else {
            kR *= 0.643;
            f = libm_pow(M_E, (-kR * kR / 2.0));
        }
        table[k2] = f;
    }
    return SHQ_OK;
}

extern "C" int shq_uvbg_keep_grids(shq_context *ctx, int enable)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    ctx->uvbg_keep = enable != 0;
    if(!ctx->uvbg_keep) {
        std::vector<float>().swap(ctx->uvbg_j21);
        std::vector<float>().swap(ctx->uvbg_xhi);
        ctx->uvbg_n = 0;
    }
    return SHQ_OK;
}

extern "C" int shq_uvbg_download_grids(shq_context *ctx, int Nmesh, float *J21, float *xHI)
{
    SHQ_CHECK(ctx && J21 && xHI, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(ctx->uvbg_n > 0, SHQ_ERR_STATE, "uvbg_download_grids: no grids kept (shq_uvbg_keep_grids(ctx, 1) before the call)");
    SHQ_CHECK(Nmesh == ctx->uvbg_n, SHQ_ERR_INVALID, "uvbg_download_grids: the kept grids are %d^3, not %d^3", ctx->uvbg_n, Nmesh);
    memcpy(J21, ctx->uvbg_j21.data(), sizeof(float) * ctx->uvbg_j21.size());
    memcpy(xHI, ctx->uvbg_xhi.data(), sizeof(float) * ctx->uvbg_xhi.size());
    return SHQ_OK;
}

extern "C" int shq_uvbg_phase_ms(shq_context *ctx, double ms[4])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 4; i++)
        ms[i] = ctx->uvbg_ms[i];
    return SHQ_OK;
}

extern "C" int shq_uvbg_calculate(shq_context *ctx, const shq_uvbg_params *p, const shq_uvbg_cosmo *cp, const shq_part_view *parts,
                                  double *fesc, const double *sfr, double *local_J21, double *zreion, shq_uvbg_result *result)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && p && cp && parts && fesc && local_J21 && zreion && result, SHQ_ERR_INVALID, "uvbg: null argument");
    const int use_sfr = p->ReionUseParticleSFR ? 1 : 0;
    SHQ_CHECK(!use_sfr || sfr, SHQ_ERR_INVALID, "uvbg: ReionUseParticleSFR needs the Sfr array");
    const int N = p->UVBGdim;
    SHQ_CHECK(N >= 4 && N % 2 == 0 && (long long) N * N * N < (1ll << 31), SHQ_ERR_INVALID,
              "uvbg: UVBGdim must be even, >= 4 and UVBGdim^3 an int (divide_by_ncell), got %d", N);
    SHQ_CHECK(p->BoxSize > 0 && cp->Time > 0 && p->ReionDeltaRFactor > 0, SHQ_ERR_INVALID, "uvbg: BoxSize, Time and ReionDeltaRFactor must be > 0");
    SHQ_CHECK(p->ReionFilterType >= 0 && p->ReionFilterType <= 2, SHQ_ERR_INVALID, "ReionFilterType type %d is undefined!", p->ReionFilterType);
    SHQ_CHECK(p->RtoMFilterType == 0 || p->RtoMFilterType == 1, SHQ_ERR_INVALID, "Unrecognised RtoM filter (%d).", p->RtoMFilterType);
    const long long n = parts->numpart;
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || parts->base), SHQ_ERR_INVALID, "uvbg: bad particle view");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_CHECK(parts_resident(ctx, parts) || (parts->off_pos != SHQ_NOFIELD && parts->off_mass != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD),
              SHQ_ERR_INVALID, "uvbg: the particle view needs Pos, Mass and Type");
    /* the radius schedule of petapm_reion_c2r (petapm.cpp:536-606) */
    std::vector<double> radii;
    const double cell = p->BoxSize / N; /* pm->CellSize, petapm.cpp:205 */
    {
        double R = fmin(p->ReionRBubbleMax, p->BoxSize);
        int last = 0, count = 0;
        while(!last) {
            count++;
            if(R / p->ReionDeltaRFactor < p->ReionRBubbleMin || R / p->ReionDeltaRFactor < cell || count > UVBG_MAX_R_ITERATIONS) {
                last = 1;
                R = cell;
            }
            radii.push_back(R);
            R = R / p->ReionDeltaRFactor;
        }
    }
    /* every radius' filter table (shq_uvbg_filter_table: glibc's sinf / cosf / powf per k2, 0.1 s on one core for 42 radii at Nmesh 512),
     * made by host threads beside the staging and the device's first half; the last step is unfiltered: one entry, fac_mask 0 */
    const int nr = (int) radii.size();
    const size_t ntab = 3 * (size_t) (N / 2) * (N / 2) + 1;
    std::vector<double> tabs((size_t) nr * ntab);
    tabs[(size_t) (nr - 1) * ntab] = 1.0;
    constexpr int NTHR = 8;
    std::future<void> tables[NTHR];
    for(int j = 0; j < NTHR; j++)
        tables[j] = std::async(std::launch::async, [&, j]() {
            for(int r = j; r + 1 < nr; r += NTHR)
                (void) shq_uvbg_filter_table(p->ReionFilterType, N, p->BoxSize, radii[r], tabs.data() + (size_t) r * ntab);
        });
    hipStream_t s = ctx->stream;
    CallScope sc(ctx, "uvbg");
    SHQ_TRY(sc.mark(s));

    /* ---- particles: the resident set, or staged into the call's own buffers */
    const size_t np = (size_t) (n > 0 ? n : 1);
    const double4 *d_posm;
    const uint8_t *d_flags;
    SHQ_TRY(stage_part_view(ctx, sc, parts, true, &d_posm, &d_flags));
    double *d_fesc, *d_sfr = nullptr, *d_lj, *d_zr, *d_part, *d_sums;
    int *d_neg;
    const int pblocks = (int) std::min(1024u, nblk(n, UV_T));
    SHQ_TRY(sc.alloc(&d_fesc, np));
    SHQ_TRY(sc.alloc(&d_lj, np));
    SHQ_TRY(sc.alloc(&d_zr, np));
    SHQ_TRY(sc.alloc(&d_part, 3 * (size_t) std::max(pblocks, UV_CELL_BLOCKS)));
    SHQ_TRY(sc.alloc(&d_sums, 3));
    SHQ_TRY(sc.alloc(&d_neg, 1));
    if(use_sfr)
        SHQ_TRY(sc.alloc(&d_sfr, np));
    if(n > 0) {
        SHQ_HIP(hipMemcpyAsync(d_fesc, fesc, sizeof(double) * n, hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemcpyAsync(d_lj, local_J21, sizeof(double) * n, hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemcpyAsync(d_zr, zreion, sizeof(double) * n, hipMemcpyHostToDevice, s));
        if(use_sfr)
            SHQ_HIP(hipMemcpyAsync(d_sfr, sfr, sizeof(double) * n, hipMemcpyHostToDevice, s));
    }
    SHQ_HIP(hipMemsetAsync(d_neg, 0, sizeof(int), s));

    /* ---- init_particle_uvbg and the fields' sums */
    const double fesc_unit_conv = cp->UnitMass_in_g / UVBG_SOLAR_MASS / 1e10 / cp->HubbleParam;
    uvbg_fesc_kernel<<<dim3(pblocks), dim3(UV_T), 0, s>>>(n, d_posm, d_flags, d_fesc, d_sfr, use_sfr, p->EscapeFractionNorm,
                                                          p->EscapeFractionScaling, fesc_unit_conv, d_part, d_neg);
    uvbg_sum_kernel<<<dim3(1), dim3(UV_T), 0, s>>>(d_part, pblocks, d_sums);
    SHQ_HIP(hipGetLastError());
    double sums[3];
    int neg = 0;
    SHQ_HIP(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipMemcpyAsync(&neg, d_neg, sizeof(int), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    SHQ_CHECK(neg == 0, SHQ_ERR_INVALID, "negative escape fraction?");
    SHQ_CHECK(isfinite(sums[0]) && isfinite(sums[1]) && isfinite(sums[2]), SHQ_ERR_INVALID, "uvbg: non-finite mass, f_esc or Sfr");

    /* ---- meshes: per field the deposit / kept spectrum and the real mesh of the radius, one scratch mesh; the grids */
    const int nf = use_sfr ? 3 : 2;
    Fft3dRoute route = fft3d_route(N);
    const bool bespoke = route.bespoke; /* this side is uvbg's own: the transposing pipeline with the filter in it */
    const int zp = route.zp;
    const size_t padded = route.padded, dense = (size_t) N * N * N;
    double *spec[3] = {nullptr, nullptr, nullptr}, *real[3] = {nullptr, nullptr, nullptr}, *scratch = nullptr, *d_tw = nullptr;
    for(int f = 0; f < nf; f++) {
        SHQ_TRY(sc.alloc(&spec[f], padded));
        SHQ_TRY(sc.alloc(&real[f], padded));
        SHQ_HIP(hipMemsetAsync(spec[f], 0, sizeof(double) * padded, s));
    }
    if(bespoke) {
        SHQ_TRY(sc.alloc(&scratch, padded));
        SHQ_TRY(sc.alloc(&d_tw, 2 * (size_t) N));
        SHQ_TRY(shq_fft3d_fill_twiddles(N, d_tw));
    }
    SHQ_TRY(route_plans(sc, route, true, true));
    float *d_j21, *d_xhi;
    SHQ_TRY(sc.alloc(&d_j21, dense));
    SHQ_TRY(sc.alloc(&d_xhi, dense));
    SHQ_HIP(hipMemsetAsync(d_j21, 0, sizeof(float) * dense, s));
    uvbg_fill_kernel<<<dim3(1024), dim3(UV_T), 0, s>>>(d_xhi, dense, 1.0f);

    /* ---- deposit: each field with its own scale 2^(61 - e), its sum < 2^e (the PM's choice, shq_particles_upload) */
    double scale[3], inv_scale[3];
    for(int f = 0; f < 3; f++) {
        int ex = 0;
        (void) frexp(sums[f] > 0 ? sums[f] : 1.0, &ex);
        scale[f] = ldexp(1.0, 61 - ex);
        inv_scale[f] = ldexp(1.0, ex - 61);
    }
    if(n > 0)
        uvbg_deposit_kernel<<<dim3(nblk(n, UV_T)), dim3(UV_T), 0, s>>>(
            n, d_posm, d_flags, d_fesc, d_sfr, use_sfr, N, zp, cell, scale[0], scale[1], scale[2], (unsigned long long *) spec[0],
            (unsigned long long *) spec[1], use_sfr ? (unsigned long long *) spec[2] : nullptr);
    SHQ_HIP(hipGetLastError());

    /* ---- forward transforms, the spectra kept for the whole radius loop */
    const int ncell = N * N * N; /* divide_by_ncell's int total_n_cells */
    for(int f = 0; f < nf; f++) {
        if(bespoke) {
            shq_fft_opts o;
            o.tw = d_tw;
            SHQ_TRY(shq_fft3d_run_transposed(ctx, spec[f], scratch, N, zp, SHQ_FFT_T_FORWARD, true, inv_scale[f], nullptr, 0, 0, o));
        } else {
            mesh_convert_i64_kernel<<<dim3(2048), dim3(UV_T), 0, s>>>(spec[f], padded, inv_scale[f]);
            SHQ_TRY(route_hipfft_forward(sc, route, spec[f]));
        }
    }
    SHQ_TRY(sc.mark(s)); /* ev[1]: deposited and transformed */

    /* ---- the filter tables from the host threads */
    for(auto &t : tables)
        t.wait();
    double *d_tabs;
    SHQ_TRY(sc.alloc(&d_tabs, tabs.size()));
    SHQ_HIP(hipMemcpyAsync(d_tabs, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice, s));

    /* ---- reion_loop_pm's constants (uvbg.cpp:336-370), in the reference's operation order */
    const double redshift = 1.0 / cp->Time - 1.;
    const double Y_He = 1.0 - UVBG_HYDROGEN_MASSFRAC;
    const double BaryonFrac = cp->OmegaBaryon / cp->Omega0;
    const double ReionEfficiency = 1.0 / BaryonFrac * p->ReionNionPhotPerBary / (1.0 - 0.75 * Y_He);
    const double tot_n_cells = N * N * N;
    const double pixel_volume = cell * cell * cell;
    const double deltax_conv_factor = tot_n_cells / (cp->RhoCrit * cp->Omega0 * p->BoxSize * p->BoxSize * p->BoxSize);
    const double hubble_time = 1 / (cp->hubble * cp->HubbleParam);
    UvbgCell c;
    c.deltax_conv = deltax_conv_factor;
    c.pixel_volume = pixel_volume;
    c.inv_eff = 1.0 / ReionEfficiency;
    c.eff = ReionEfficiency;
    c.sfr_mass_unit = cp->UnitMass_in_g / UVBG_SOLAR_MASS;
    c.sfr_time_unit = cp->UnitTime_in_s / UVBG_SEC_PER_YEAR;
    c.sfr_timescale = p->ReionSFRTimescale * hubble_time;
    c.use_sfr = use_sfr;
    const int cblocks = (int) std::min<long long>(UV_CELL_BLOCKS, ((long long) dense + UV_T - 1) / UV_T);
    for(int r = 0; r < nr; r++) {
        const double R = radii[r];
        const bool last = r == nr - 1;
        const double *fac = d_tabs + (size_t) r * ntab;
        const int mask = last ? 0 : -1;
        for(int f = 0; f < nf; f++) {
            if(bespoke) {
                shq_fft_opts o;
                o.tw = d_tw;
                o.out = real[f];
                o.modefac = fac;
                o.fac_mask = mask;
                o.ncell = ncell;
                SHQ_TRY(shq_fft3d_run_transposed(ctx, spec[f], scratch, N, zp, SHQ_FFT_T_FILTER, false, 1.0, nullptr, 0, 0, o));
            } else {
                uvbg_filter_kernel<<<dim3(2048), dim3(UV_T), 0, s>>>((const double2 *) spec[f], (double2 *) real[f], N, fac, mask, ncell);
                SHQ_TRY(route_hipfft_inverse(sc, route, real[f]));
            }
        }
        c.R = R;
        c.last = last ? 1 : 0;
        c.rtom = p->RtoMFilterType == 0 ? (4.0 / 3.0) * M_PI * libm_pow(R, 3) * (cp->Omega0 * cp->RhoCrit)
                                        : libm_pow(2 * M_PI, 1.5) * cp->Omega0 * cp->RhoCrit * libm_pow(R, 3);
        c.J21c = (1.0 + redshift) * (1.0 + redshift) / (4.0 * M_PI) * p->AlphaUV * UVBG_PLANCK * 1e21 * R * cp->UnitLength_in_cm *
                 p->ReionNionPhotPerBary / UVBG_PROTONMASS * cp->UnitMass_in_g / libm_pow(cp->UnitLength_in_cm, 3) / cp->UnitTime_in_s;
        uvbg_cell_kernel<<<dim3(cblocks), dim3(UV_T), 0, s>>>(real[0], real[1], use_sfr ? real[2] : real[1], N, zp, c, d_j21, d_xhi, d_part);
        SHQ_HIP(hipGetLastError());
    }
    uvbg_sum_kernel<<<dim3(1), dim3(UV_T), 0, s>>>(d_part, cblocks, d_sums);
    SHQ_TRY(sc.mark(s)); /* ev[2]: the radius loop */

    /* ---- readout_J21, then the particles' results */
    if(n > 0)
        uvbg_readout_kernel<<<dim3(nblk(n, UV_T)), dim3(UV_T), 0, s>>>(n, d_posm, d_flags, d_j21, N, cell, 1 / cp->Time - 1,
                                                                                           d_lj, d_zr);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, s));
    if(n > 0) {
        SHQ_HIP(hipMemcpyAsync(fesc, d_fesc, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipMemcpyAsync(local_J21, d_lj, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipMemcpyAsync(zreion, d_zr, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    }
    if(ctx->uvbg_keep) {
        ctx->uvbg_n = 0;
        ctx->uvbg_j21.resize(dense);
        ctx->uvbg_xhi.resize(dense);
        SHQ_HIP(hipMemcpyAsync(ctx->uvbg_j21.data(), d_j21, sizeof(float) * dense, hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipMemcpyAsync(ctx->uvbg_xhi.data(), d_xhi, sizeof(float) * dense, hipMemcpyDeviceToHost, s));
    }
    SHQ_TRY(sc.mark(s)); /* ev[3]: read out and downloaded */
    SHQ_HIP(hipStreamSynchronize(s));
    if(ctx->uvbg_keep)
        ctx->uvbg_n = N;
    result->volume_weighted_global_xHI = sums[0] / (double) (int64_t) dense;
    result->mass_weighted_global_xHI = sums[1] / sums[2];
    result->nradii = nr;
    result->pad_ = 0;
    const int from[4] = {0, 1, 2, 0}, to[4] = {1, 2, 3, 3};
    for(int i = 0; i < 4; i++)
        ctx->uvbg_ms[i] = sc.ms(from[i], to[i]);
    return SHQ_OK;
}
