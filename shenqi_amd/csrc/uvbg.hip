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
 *
 * Several ranks: the same phases as entry points of their own on a rank's x-slab (shq_uvbg_slab_*, at the end of the file), with the
 * caller's transposes between them (shenqi_amd/dist.py, DistUVBG).  The particle and cell kernels are the ones above with a plane
 * window: one rank is the window (plane 0, N planes).
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
 * |Sfr f_esc| (Type 0) that pick the deposit scales.  The Type is pflags >> tshift: 4 for the context's flag bytes, 0 for plain types. */
__global__ __launch_bounds__(UV_T) void uvbg_fesc_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                         int tshift, double *fesc, const double *__restrict__ sfr, int use_sfr, double norm,
                                                         double scaling, double conv, double *part, int *neg)
{
    __shared__ double lds[UV_T];
    double s0 = 0, s1 = 0, s2 = 0;
    for(long long i = (long long) blockIdx.x * UV_T + threadIdx.x; i < n; i += (long long) gridDim.x * UV_T) {
        const int t = pflags[i] >> tshift;
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

/* put_particle_to_mesh / put_star_to_mesh / put_sfr_to_mesh (petapm.cpp:1304-1328) in one pass: weight * Mass [* f_esc] in fixed point,
 * into the window [nxalloc][N][zp] of each mesh whose plane 0 is the global plane xshift (one rank: 0 and N) */
__global__ __launch_bounds__(UV_T) void uvbg_deposit_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                            int tshift, const double *__restrict__ fesc, const double *__restrict__ sfr,
                                                            int use_sfr, int N, int zp, double cell, double sc0, double sc1, double sc2,
                                                            unsigned long long *m0, unsigned long long *m1, unsigned long long *m2, int xshift,
                                                            int nxalloc, int *oob)
{
    const long long i = (long long) blockIdx.x * UV_T + threadIdx.x;
    if(i >= n)
        return;
    const double4 p = posm[i];
    const int t = pflags[i] >> tshift;
    const bool star = t == 4, gas = t == 0 && use_sfr;
    const double f = (star || gas) ? fesc[i] : 0.0;
    const double s = gas ? sfr[i] : 0.0;
    int ic[3];
    double res[3];
    cic_cell3(p.x, p.y, p.z, cell, N, ic, res);
    cic_corners<true>(ic, res, N, zp, [&](int, size_t lin, double w) {
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
    }, xshift, nxalloc, oob);
}

/* hipFFT route: divide_by_ncell then filter_pm on the kept [x][y][z'] half spectrum, into the field's mesh; of a y-slab the rows
 * y0 .. y0 + nyl - 1, [x][nyl][z'] (one rank: 0 and N) */
__global__ void uvbg_filter_kernel(const double2 *__restrict__ spec, double2 *out, int N, int y0, int nyl, const double *__restrict__ fac,
                                   int fac_mask, int ncell)
{
#pragma clang fp contract(off)
    const int Nc = N / 2 + 1;
    const size_t n = (size_t) N * nyl * Nc;
    const double nc = (double) ncell;
    for(size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        const size_t row = i / Nc;
        const int z = (int) (i - row * Nc), x = (int) (row / nyl), y = y0 + (int) (row - (size_t) x * nyl);
        const int kx = x <= N / 2 ? x : x - N, ky = y <= N / 2 ? y : y - N;
        const double T = fac[(kx * kx + ky * ky + z * z) & fac_mask];
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
 * partial ionisations and the block's sums of xHI, xHI density_over_mean and density_over_mean.  The cells are `nplanes` planes: of the
 * meshes (pitch zp) from buffer plane xoff on, of the dense float grids from their first (one rank: N planes, xoff 0) */
__global__ __launch_bounds__(UV_T) void uvbg_cell_kernel(const double *__restrict__ mass, const double *__restrict__ star,
                                                         const double *__restrict__ sfr, int N, int zp, int nplanes, int xoff, const UvbgCell c,
                                                         float *J21, float *xHI, double *part)
{
#pragma clang fp contract(off)
    __shared__ double lds[UV_T];
    const long long ncell = (long long) nplanes * N * N;
    double s0 = 0, s1 = 0, s2 = 0;
    for(long long g = (long long) blockIdx.x * UV_T + threadIdx.x; g < ncell; g += (long long) gridDim.x * UV_T) {
        const long long row = g / N;
        const size_t m = (size_t) (row + (long long) xoff * N) * zp + (size_t) (g - row * N);
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
 * included, in connection order.  J21 is the window [nxalloc][N][N] whose plane 0 is the global plane xshift (one rank: 0 and N) */
__global__ __launch_bounds__(UV_T) void uvbg_readout_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                            int tshift, const float *__restrict__ J21, int N, double cell, double zre_now,
                                                            double *local_J21, double *zreion, int xshift, int nxalloc, int *oob)
{
    const long long i = (long long) blockIdx.x * UV_T + threadIdx.x;
    if(i >= n || (pflags[i] >> tshift) != 0)
        return;
    const double4 p = posm[i];
    int ic[3];
    double res[3];
    cic_cell3(p.x, p.y, p.z, cell, N, ic, res);
    double lj = 0.0; /* init_particle_uvbg's reset */
    double zr = zreion[i];
    cic_corners<true>(ic, res, N, N, [&](int, size_t lin, double) { /* the grid is dense [.][N][N]; the weight plays no part */
        const double v = (double) J21[lin];
        if(v > lj) {
            lj = v;
            if(zr == -1)
                zr = zre_now;
        }
    }, xshift, nxalloc, oob);
    local_J21[i] = lj;
    zreion[i] = zr;
}

/* the radius schedule of petapm_reion_c2r (petapm.cpp:536-606); cell = pm->CellSize, petapm.cpp:205 */
std::vector<double> uvbg_radii(const shq_uvbg_params *p, double cell)
{
    std::vector<double> radii;
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
    return radii;
}

/* reion_loop_pm's constants (uvbg.cpp:336-370), in the reference's operation order */
UvbgCell uvbg_cell_constants(const shq_uvbg_params *p, const shq_uvbg_cosmo *cp, int use_sfr)
{
#pragma clang fp contract(off)
    const int N = p->UVBGdim;
    const double cell = p->BoxSize / N;
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
    return c;
}

/* ... and the ones of radius R: RtoM (uvbg.cpp:158-176) and J21_aux_constant */
void uvbg_cell_radius(UvbgCell &c, const shq_uvbg_params *p, const shq_uvbg_cosmo *cp, double R, bool last)
{
#pragma clang fp contract(off)
    const double redshift = 1.0 / cp->Time - 1.;
    c.R = R;
    c.last = last ? 1 : 0;
    c.rtom = p->RtoMFilterType == 0 ? (4.0 / 3.0) * M_PI * libm_pow(R, 3) * (cp->Omega0 * cp->RhoCrit)
                                    : libm_pow(2 * M_PI, 1.5) * cp->Omega0 * cp->RhoCrit * libm_pow(R, 3);
    c.J21c = (1.0 + redshift) * (1.0 + redshift) / (4.0 * M_PI) * p->AlphaUV * UVBG_PLANCK * 1e21 * R * cp->UnitLength_in_cm *
             p->ReionNionPhotPerBary / UVBG_PROTONMASS * cp->UnitMass_in_g / libm_pow(cp->UnitLength_in_cm, 3) / cp->UnitTime_in_s;
}

int uvbg_check_params(const shq_uvbg_params *p, const shq_uvbg_cosmo *cp)
{
    const int N = p->UVBGdim;
    SHQ_CHECK(N >= 4 && N % 2 == 0 && (long long) N * N * N < (1ll << 31), SHQ_ERR_INVALID,
              "uvbg: UVBGdim must be even, >= 4 and UVBGdim^3 an int (divide_by_ncell), got %d", N);
    SHQ_CHECK(p->BoxSize > 0 && cp->Time > 0 && p->ReionDeltaRFactor > 0, SHQ_ERR_INVALID, "uvbg: BoxSize, Time and ReionDeltaRFactor must be > 0");
    SHQ_CHECK(p->ReionFilterType >= 0 && p->ReionFilterType <= 2, SHQ_ERR_INVALID, "ReionFilterType type %d is undefined!", p->ReionFilterType);
    SHQ_CHECK(p->RtoMFilterType == 0 || p->RtoMFilterType == 1, SHQ_ERR_INVALID, "Unrecognised RtoM filter (%d).", p->RtoMFilterType);
    return SHQ_OK;
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
    SHQ_TRY(uvbg_check_params(p, cp));
    const long long n = parts->numpart;
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || parts->base), SHQ_ERR_INVALID, "uvbg: bad particle view");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_CHECK(parts_resident(ctx, parts) || (parts->off_pos != SHQ_NOFIELD && parts->off_mass != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD),
              SHQ_ERR_INVALID, "uvbg: the particle view needs Pos, Mass and Type");
    const double cell = p->BoxSize / N; /* pm->CellSize, petapm.cpp:205 */
    const std::vector<double> radii = uvbg_radii(p, cell);
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
    int *d_neg; /* [0] a negative escape fraction, [1] a CIC corner outside the mesh window (cannot happen on one rank) */
    const int pblocks = (int) std::min(1024u, nblk(n, UV_T));
    SHQ_TRY(sc.alloc(&d_fesc, np));
    SHQ_TRY(sc.alloc(&d_lj, np));
    SHQ_TRY(sc.alloc(&d_zr, np));
    SHQ_TRY(sc.alloc(&d_part, 3 * (size_t) std::max(pblocks, UV_CELL_BLOCKS)));
    SHQ_TRY(sc.alloc(&d_sums, 3));
    SHQ_TRY(sc.alloc(&d_neg, 2));
    if(use_sfr)
        SHQ_TRY(sc.alloc(&d_sfr, np));
    if(n > 0) {
        SHQ_HIP(hipMemcpyAsync(d_fesc, fesc, sizeof(double) * n, hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemcpyAsync(d_lj, local_J21, sizeof(double) * n, hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemcpyAsync(d_zr, zreion, sizeof(double) * n, hipMemcpyHostToDevice, s));
        if(use_sfr)
            SHQ_HIP(hipMemcpyAsync(d_sfr, sfr, sizeof(double) * n, hipMemcpyHostToDevice, s));
    }
    SHQ_HIP(hipMemsetAsync(d_neg, 0, 2 * sizeof(int), s));

    /* ---- init_particle_uvbg and the fields' sums */
    const double fesc_unit_conv = cp->UnitMass_in_g / UVBG_SOLAR_MASS / 1e10 / cp->HubbleParam;
    uvbg_fesc_kernel<<<dim3(pblocks), dim3(UV_T), 0, s>>>(n, d_posm, d_flags, 4, d_fesc, d_sfr, use_sfr, p->EscapeFractionNorm,
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
            n, d_posm, d_flags, 4, d_fesc, d_sfr, use_sfr, N, zp, cell, scale[0], scale[1], scale[2], (unsigned long long *) spec[0],
            (unsigned long long *) spec[1], use_sfr ? (unsigned long long *) spec[2] : nullptr, 0, N, d_neg + 1);
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

    /* ---- reion_loop_pm's constants (uvbg.cpp:336-370) */
    UvbgCell c = uvbg_cell_constants(p, cp, use_sfr);
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
                uvbg_filter_kernel<<<dim3(2048), dim3(UV_T), 0, s>>>((const double2 *) spec[f], (double2 *) real[f], N, 0, N, fac, mask, ncell);
                SHQ_TRY(route_hipfft_inverse(sc, route, real[f]));
            }
        }
        uvbg_cell_radius(c, p, cp, R, last);
        uvbg_cell_kernel<<<dim3(cblocks), dim3(UV_T), 0, s>>>(real[0], real[1], use_sfr ? real[2] : real[1], N, zp, N, 0, c, d_j21, d_xhi,
                                                              d_part);
        SHQ_HIP(hipGetLastError());
    }
    uvbg_sum_kernel<<<dim3(1), dim3(UV_T), 0, s>>>(d_part, cblocks, d_sums);
    SHQ_TRY(sc.mark(s)); /* ev[2]: the radius loop */

    /* ---- readout_J21, then the particles' results */
    if(n > 0)
        uvbg_readout_kernel<<<dim3(nblk(n, UV_T)), dim3(UV_T), 0, s>>>(n, d_posm, d_flags, 4, d_j21, N, cell, 1 / cp->Time - 1, d_lj, d_zr, 0,
                                                                       N, d_neg + 1);
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

/* ---- the same phases on a rank's x-slab (several ranks: shenqi_amd/dist.py, DistUVBG) -------------------------------------------
 * Every pointer named d_ is device memory of the caller (torch tensors).  d_posm = double[n][4] rows (x, y, z, m), d_types = uint8[n]
 * plain Types.  A mesh field is one buffer [nalloc][N][zp] doubles, in turn the int64 deposit, the (y, z) half spectrum and the real
 * mesh of a radius; the slab's first own plane is buffer plane xoff (shq_pm_slab2_*'s window).  None of these calls reads or writes
 * the PM's state: the deposit scales are arguments, the twiddles and tables are the context's uvbg ones. */
namespace {

int uvbg_slab_scratch(shq_context *ctx, size_t nblocks)
{
    SHQ_TRY(ctx->uvbg_part.reserve(3 * nblocks + 3)); /* the blocks' partial sums, then the three totals */
    return slab_flag_reset(ctx, ctx->uvbg_flag, 2); /* [0] a negative escape fraction, [1] a particle outside the slab's window */
}

bool uvbg_window_ok(int N, int plane0, int nplanes, int xoff, int nalloc)
{
    return nplanes > 0 && nplanes <= N && plane0 >= 0 && plane0 < N && xoff >= 0 && xoff + nplanes <= nalloc && nalloc <= N + 8;
}

} // namespace

extern "C" int shq_uvbg_slab_pitch(int UVBGdim) { return slab_pitch(UVBGdim); }

extern "C" int shq_uvbg_slab_fesc(shq_context *ctx, const shq_uvbg_params *p, const shq_uvbg_cosmo *cp, const void *d_posm, const void *d_types,
                                  int64_t n, void *d_fesc, const void *d_sfr, double sums[3], int *negative)
{
    SHQ_CHECK(ctx && p && cp && sums && negative, SHQ_ERR_INVALID, "uvbg_slab_fesc: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_posm && d_types && d_fesc)), SHQ_ERR_INVALID, "uvbg_slab_fesc: bad particle arrays");
    const int use_sfr = p->ReionUseParticleSFR ? 1 : 0;
    SHQ_CHECK(!use_sfr || n == 0 || d_sfr, SHQ_ERR_INVALID, "uvbg: ReionUseParticleSFR needs the Sfr array");
    SHQ_TRY(uvbg_check_params(p, cp));
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int pblocks = (int) std::min(1024u, nblk(n, UV_T));
    SHQ_TRY(uvbg_slab_scratch(ctx, (size_t) pblocks));
    double *part = ctx->uvbg_part.ptr, *tot = part + 3 * (size_t) pblocks;
    const double fesc_unit_conv = cp->UnitMass_in_g / UVBG_SOLAR_MASS / 1e10 / cp->HubbleParam;
    uvbg_fesc_kernel<<<dim3(pblocks), dim3(UV_T), 0, s>>>(n, (const double4 *) d_posm, (const uint8_t *) d_types, 0, (double *) d_fesc,
                                                          (const double *) d_sfr, use_sfr, p->EscapeFractionNorm, p->EscapeFractionScaling,
                                                          fesc_unit_conv, part, ctx->uvbg_flag.ptr);
    uvbg_sum_kernel<<<dim3(1), dim3(UV_T), 0, s>>>(part, pblocks, tot);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(sums, tot, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipMemcpyAsync(negative, ctx->uvbg_flag.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    SHQ_CHECK(isfinite(sums[0]) && isfinite(sums[1]) && isfinite(sums[2]), SHQ_ERR_INVALID, "uvbg: non-finite mass, f_esc or Sfr");
    return SHQ_OK;
}

/* exps[f] = e: field f is deposited with the scale 2^(61 - e), the frexp exponent of its sum over ALL ranks (the one-rank call's
 * choice), so that every rank count deposits the same integers.  Zeroes the buffers first; d_m2 only with ReionUseParticleSFR. */
extern "C" int shq_uvbg_slab_deposit(shq_context *ctx, const shq_uvbg_params *p, const void *d_posm, const void *d_types, int64_t n,
                                     const void *d_fesc, const void *d_sfr, const int exps[3], int plane0, int nplanes, int xoff, int nalloc,
                                     int nghost, void *d_m0, void *d_m1, void *d_m2)
{
    SHQ_CHECK(ctx && p && exps && d_m0 && d_m1, SHQ_ERR_INVALID, "uvbg_slab_deposit: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_posm && d_types && d_fesc)), SHQ_ERR_INVALID, "uvbg_slab_deposit: bad particle arrays");
    const int use_sfr = p->ReionUseParticleSFR ? 1 : 0;
    SHQ_CHECK(!use_sfr || (d_m2 && (n == 0 || d_sfr)), SHQ_ERR_INVALID, "uvbg: ReionUseParticleSFR needs the Sfr array and a third mesh");
    const int N = p->UVBGdim;
    SHQ_CHECK(N >= 4 && N % 2 == 0, SHQ_ERR_INVALID, "uvbg_slab_deposit: bad mesh size %d", N);
    const int zp = fft3d_route(N).zp; /* the slab pitch, or N + 2 on the route without a bespoke transform */
    SHQ_CHECK(uvbg_window_ok(N, plane0, nplanes, xoff, nalloc) && nghost == 1 && p->BoxSize > 0, SHQ_ERR_INVALID, "uvbg_slab_deposit: bad slab geometry");
    const int nfit = nplanes == N ? N : xoff + nplanes + nghost;
    SHQ_CHECK(nfit <= nalloc, SHQ_ERR_INVALID, "uvbg_slab_deposit: no room for the deposit ghost plane");
    for(int f = 0; f < 3; f++)
        SHQ_CHECK(exps[f] > -900 && exps[f] < 900, SHQ_ERR_INVALID, "uvbg_slab_deposit: bad scale exponent %d", exps[f]);
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHQ_TRY(uvbg_slab_scratch(ctx, 1));
    const size_t cnt = sizeof(double) * (size_t) nalloc * N * zp;
    SHQ_HIP(hipMemsetAsync(d_m0, 0, cnt, s));
    SHQ_HIP(hipMemsetAsync(d_m1, 0, cnt, s));
    if(use_sfr)
        SHQ_HIP(hipMemsetAsync(d_m2, 0, cnt, s));
    if(n > 0)
        uvbg_deposit_kernel<<<dim3(nblk(n, UV_T)), dim3(UV_T), 0, s>>>(
            n, (const double4 *) d_posm, (const uint8_t *) d_types, 0, (const double *) d_fesc, (const double *) d_sfr, use_sfr, N, zp,
            p->BoxSize / N, ldexp(1.0, 61 - exps[0]), ldexp(1.0, 61 - exps[1]), ldexp(1.0, 61 - exps[2]), (unsigned long long *) d_m0,
            (unsigned long long *) d_m1, use_sfr ? (unsigned long long *) d_m2 : nullptr, plane0 - xoff, nfit, ctx->uvbg_flag.ptr + 1);
    SHQ_HIP(hipGetLastError());
    int oob;
    SHQ_TRY(slab_flag_read(ctx, ctx->uvbg_flag.ptr + 1, &oob));
    SHQ_CHECK(!oob, SHQ_ERR_INVALID, "uvbg_slab_deposit: a particle lies outside this rank's slab (planes %d .. %d)", plane0, plane0 + nplanes - 1);
    return SHQ_OK;
}

/* shq_pm_slab2_fft_yz(_packed) with the scale as an argument: direction 0 takes the int64 planes of a field deposited with exponent
 * `exp` (worth 2^(exp - 61) per unit) to the (y, z) half spectrum, direction 1 goes back to real space.  d_packed (NULL: in place) is
 * the all-to-all buffer [nranks][nplanes][N / nranks][zp / 2] complex of shq_pm_slab2_fft_yz_packed. */
extern "C" int shq_uvbg_slab_fft_yz(shq_context *ctx, int UVBGdim, void *d_planes, int nplanes, int direction, int exp, void *d_packed, int nranks)
{
    return slab_fft_yz(ctx, "uvbg_slab_fft_yz", &shq_context::uvbg_tw, &shq_context::uvbg_tw_n, UVBGdim, d_planes, nplanes, direction, exp, d_packed, nranks);
}

/* the X forward of the y-slab [N][nyl][zp / 2] complex the all-to-all delivers, in place: the spectrum kept for the radius loop */
extern "C" int shq_uvbg_slab_xforward(shq_context *ctx, int UVBGdim, void *d_spec, int y0, int nyl)
{
    SHQ_CHECK(ctx && d_spec, SHQ_ERR_INVALID, "uvbg_slab_xforward: null argument");
    const int N = UVBGdim, zp = shq_uvbg_slab_pitch(N);
    SHQ_CHECK(zp > 0, SHQ_ERR_INVALID, "uvbg_slab_xforward: mesh size %d has no bespoke FFT", N);
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N, SHQ_ERR_INVALID, "uvbg_slab_xforward: bad slab geometry");
    SHQ_HIP(hipSetDevice(ctx->device));
    shq_fft_opts o;
    SHQ_TRY(slab_twiddles(ctx, ctx->uvbg_tw, ctx->uvbg_tw_n, N, &o.tw));
    o.nslab = nyl;
    o.y0 = y0;
    return shq_fft3d_run(ctx, (double *) d_spec, N, zp, SHQ_FFT_X_FORWARD_SUMS, false, 1.0, nullptr, 0, 0, o);
}

/* The filter tables of the radius loop, made on the host (shq_uvbg_filter_table) and kept on the device until the next call: one per
 * radius but the last, which is unfiltered.  Every rank makes the same tables. */
extern "C" int shq_uvbg_slab_tables(shq_context *ctx, int filter_type, int UVBGdim, double BoxSize, const double *radii, int nradii)
{
    SHQ_CHECK(ctx && radii && nradii >= 1 && nradii <= UVBG_MAX_R_ITERATIONS + 1, SHQ_ERR_INVALID, "uvbg_slab_tables: bad arguments");
    const int N = UVBGdim;
    SHQ_CHECK(N >= 4 && N % 2 == 0, SHQ_ERR_INVALID, "uvbg_slab_tables: bad mesh size %d", N);
    SHQ_HIP(hipSetDevice(ctx->device));
    const size_t ntab = 3 * (size_t) (N / 2) * (N / 2) + 1;
    std::vector<double> tabs((size_t) nradii * ntab);
    tabs[(size_t) (nradii - 1) * ntab] = 1.0;
    constexpr int NTHR = 8;
    std::future<int> jobs[NTHR];
    for(int j = 0; j < NTHR; j++)
        jobs[j] = std::async(std::launch::async, [&, j]() {
            int rc = SHQ_OK;
            for(int r = j; r + 1 < nradii; r += NTHR)
                if(shq_uvbg_filter_table(filter_type, N, BoxSize, radii[r], tabs.data() + (size_t) r * ntab) != SHQ_OK)
                    rc = SHQ_ERR_INVALID;
            return rc;
        });
    int rc = SHQ_OK;
    for(auto &j : jobs)
        if(j.get() != SHQ_OK)
            rc = SHQ_ERR_INVALID;
    SHQ_CHECK(rc == SHQ_OK, SHQ_ERR_INVALID, "uvbg_slab_tables: bad filter arguments (filter type %d)", filter_type);
    ctx->uvbg_tabs_n = 0;
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* a filter pass may still read the previous tables */
    SHQ_TRY(ctx->uvbg_tabs.reserve(tabs.size()));
    SHQ_HIP(hipMemcpy(ctx->uvbg_tabs.ptr, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice));
    ctx->uvbg_tabs_n = N;
    ctx->uvbg_tabs_nr = nradii;
    return SHQ_OK;
}

/* The filter pass of radius `r` of the tables (the last one: unfiltered) on the kept spectrum d_spec = [N][nyl][zp / 2] complex:
 * (v / ncell) T[k2], then the X inverse, stored into d_out of the same shape.  d_spec is only read. */
extern "C" int shq_uvbg_slab_xfilter(shq_context *ctx, int UVBGdim, const void *d_spec, void *d_out, int y0, int nyl, int r)
{
    SHQ_CHECK(ctx && d_spec && d_out && d_spec != d_out, SHQ_ERR_INVALID, "uvbg_slab_xfilter: null argument, or the pass asked to run in place");
    const int N = UVBGdim, zp = shq_uvbg_slab_pitch(N);
    SHQ_CHECK(zp > 0, SHQ_ERR_INVALID, "uvbg_slab_xfilter: mesh size %d has no bespoke FFT", N);
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N && (long long) N * N * N < (1ll << 31), SHQ_ERR_INVALID, "uvbg_slab_xfilter: bad slab geometry");
    SHQ_CHECK(ctx->uvbg_tabs_n == N && r >= 0 && r < ctx->uvbg_tabs_nr, SHQ_ERR_STATE,
              "uvbg_slab_xfilter: no table of radius %d at mesh size %d (shq_uvbg_slab_tables first)", r, N);
    SHQ_HIP(hipSetDevice(ctx->device));
    shq_fft_opts o;
    SHQ_TRY(slab_twiddles(ctx, ctx->uvbg_tw, ctx->uvbg_tw_n, N, &o.tw));
    o.nslab = nyl;
    o.y0 = y0;
    o.modefac = ctx->uvbg_tabs.ptr + (size_t) r * (3 * (size_t) (N / 2) * (N / 2) + 1);
    o.fac_mask = r == ctx->uvbg_tabs_nr - 1 ? 0 : -1;
    o.out = (double *) d_out;
    o.ncell = N * N * N;
    return shq_fft3d_run(ctx, (double *) const_cast<void *>(d_spec), N, zp, SHQ_FFT_X_FILTER, false, 1.0, nullptr, 0, 0, o);
}

/* the same filter for a mesh size without a bespoke transform, between the caller's own X transforms: d_spec = [N][nyl][N / 2 + 1]
 * complex, dense, x slowest, into d_out of the same shape (d_out may be d_spec) */
extern "C" int shq_uvbg_slab_filter(shq_context *ctx, int UVBGdim, const void *d_spec, void *d_out, int y0, int nyl, int r)
{
    SHQ_CHECK(ctx && d_spec && d_out, SHQ_ERR_INVALID, "uvbg_slab_filter: null argument");
    const int N = UVBGdim;
    SHQ_CHECK(N >= 4 && N % 2 == 0 && nyl > 0 && y0 >= 0 && y0 + nyl <= N && (long long) N * N * N < (1ll << 31), SHQ_ERR_INVALID,
              "uvbg_slab_filter: bad slab geometry");
    SHQ_CHECK(ctx->uvbg_tabs_n == N && r >= 0 && r < ctx->uvbg_tabs_nr, SHQ_ERR_STATE,
              "uvbg_slab_filter: no table of radius %d at mesh size %d (shq_uvbg_slab_tables first)", r, N);
    SHQ_HIP(hipSetDevice(ctx->device));
    const double *fac = ctx->uvbg_tabs.ptr + (size_t) r * (3 * (size_t) (N / 2) * (N / 2) + 1);
    uvbg_filter_kernel<<<dim3(2048), dim3(UV_T), 0, ctx->stream>>>((const double2 *) d_spec, (double2 *) d_out, N, y0, nyl, fac,
                                                                   r == ctx->uvbg_tabs_nr - 1 ? 0 : -1, N * N * N);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* reion_loop_pm of radius R over `nplanes` own planes: of the real meshes (pitch zp doubles: the slab pitch, or the caller's on the
 * route without a bespoke transform) from buffer plane xoff on, and of the rank's dense float planes J21 / xHI [nplanes][N][N].  last:
 * the unfiltered step; sums then receives this rank's sums of xHI, xHI density_over_mean and density_over_mean from a fixed grid. */
extern "C" int shq_uvbg_slab_cells(shq_context *ctx, const shq_uvbg_params *p, const shq_uvbg_cosmo *cp, double R, int last, const void *d_mass,
                                   const void *d_star, const void *d_sfr, int zp, int xoff, int nplanes, void *d_J21, void *d_xHI, double sums[3])
{
    SHQ_CHECK(ctx && p && cp && d_mass && d_star && d_J21 && d_xHI && (!last || sums), SHQ_ERR_INVALID, "uvbg_slab_cells: null argument");
    const int use_sfr = p->ReionUseParticleSFR ? 1 : 0;
    SHQ_CHECK(!use_sfr || d_sfr, SHQ_ERR_INVALID, "uvbg: ReionUseParticleSFR needs the Sfr mesh");
    SHQ_TRY(uvbg_check_params(p, cp));
    const int N = p->UVBGdim;
    SHQ_CHECK(nplanes > 0 && nplanes <= N && xoff >= 0 && zp >= N && R > 0, SHQ_ERR_INVALID, "uvbg_slab_cells: bad slab geometry");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const long long cells = (long long) nplanes * N * N;
    const int cblocks = (int) std::min<long long>(UV_CELL_BLOCKS, (cells + UV_T - 1) / UV_T);
    SHQ_TRY(ctx->uvbg_part.reserve(3 * (size_t) UV_CELL_BLOCKS + 3));
    double *part = ctx->uvbg_part.ptr, *tot = part + 3 * (size_t) cblocks;
    UvbgCell c = uvbg_cell_constants(p, cp, use_sfr);
    uvbg_cell_radius(c, p, cp, R, last != 0);
    uvbg_cell_kernel<<<dim3(cblocks), dim3(UV_T), 0, s>>>((const double *) d_mass, (const double *) d_star,
                                                          (const double *) (use_sfr ? d_sfr : d_star), N, zp, nplanes, xoff, c, (float *) d_J21,
                                                          (float *) d_xHI, part);
    SHQ_HIP(hipGetLastError());
    if(last) {
        uvbg_sum_kernel<<<dim3(1), dim3(UV_T), 0, s>>>(part, cblocks, tot);
        SHQ_HIP(hipGetLastError());
        SHQ_HIP(hipMemcpyAsync(sums, tot, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipStreamSynchronize(s));
    }
    return SHQ_OK;
}

/* readout_J21 for this rank's gas: d_J21 = float [nalloc][N][N], the rank's own planes from plane0 on and, for a slab with a
 * neighbour, the neighbour's first plane behind them (nalloc = nplanes + 1; nplanes = N: the whole periodic grid, nalloc = N) */
extern "C" int shq_uvbg_slab_readout(shq_context *ctx, const shq_uvbg_params *p, const shq_uvbg_cosmo *cp, const void *d_posm, const void *d_types,
                                     int64_t n, const void *d_J21, int plane0, int nplanes, int nalloc, void *d_local_J21, void *d_zreion)
{
    SHQ_CHECK(ctx && p && cp && d_J21, SHQ_ERR_INVALID, "uvbg_slab_readout: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_posm && d_types && d_local_J21 && d_zreion)), SHQ_ERR_INVALID,
              "uvbg_slab_readout: bad particle arrays");
    SHQ_TRY(uvbg_check_params(p, cp));
    const int N = p->UVBGdim;
    SHQ_CHECK(slab_window_ok(N, plane0, nplanes, nalloc), SHQ_ERR_INVALID, "uvbg_slab_readout: bad slab geometry");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHQ_TRY(uvbg_slab_scratch(ctx, 1));
    if(n > 0)
        uvbg_readout_kernel<<<dim3(nblk(n, UV_T)), dim3(UV_T), 0, s>>>(n, (const double4 *) d_posm, (const uint8_t *) d_types, 0,
                                                                       (const float *) d_J21, N, p->BoxSize / N, 1 / cp->Time - 1,
                                                                       (double *) d_local_J21, (double *) d_zreion, plane0, nalloc,
                                                                       ctx->uvbg_flag.ptr + 1);
    SHQ_HIP(hipGetLastError());
    int oob;
    SHQ_TRY(slab_flag_read(ctx, ctx->uvbg_flag.ptr + 1, &oob));
    SHQ_CHECK(!oob, SHQ_ERR_INVALID, "uvbg_slab_readout: a gas particle lies outside this rank's slab (planes %d .. %d)", plane0, plane0 + nplanes - 1);
    return SHQ_OK;
}
