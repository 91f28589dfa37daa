/* lens.hip — the lensing potential planes on the device for one rank: write_plane's compute (libgadget/plane.cpp:511-600) with
 * cutPlaneGaussianGrid / calculate_lensing_potential (libgadget/lenstools.cpp:168-319) and the PM neutrino correction
 * (cutPlanePMNeutrinoCorrection / plane_add_periodic_bilinear, plane.cpp:355-475).
 *
 * The reference makes one pass over all particles per (cut, normal) pair.  Here:
 *  - ONE particle pass bins every active particle for all planes: the two plane-axis bins are found once per axis, then every (normal,
 *    cut) whose normal-axis bin accepts the particle gets a u32 global atomic add in its count plane;
 *  - a plane kernel turns the counts into the normalised density and sums each plane's count (num_particles_plane);
 *  - one batched hipFFT 2-D r2c over all planes, a filter kernel (Poisson factor, Gaussian smoothing, zero DC, and the final
 *    cosmological scale / R^2 folded in), one batched c2r;
 *  - with a correction mesh, per requested normal one projection kernel reads the rank's x-slab once and reduces delta * overlap /
 *    Thickness along the normal axis into the Nmesh^2 planes of up to LENS_CCHUNK cuts at once, in a fixed order; the same 2-D solve at
 *    Nmesh; a bilinear-add kernel onto the R^2 planes.
 * The bins decide integer counts, so the binning arithmetic runs with contraction off: the same double operations as find_bin and
 * grid3d_ngb, bit for bit.  The bin edges and widths are made on the host with linspace's expressions.
 * The call allocates everything it uses and frees it before it returns: nothing of the context's state is touched.
 */
#include "mesh_common.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

/* physconst.h */
#define LENS_LIGHTCGS 2.99792458e10
#define LENS_CM_PER_KPC 3.085678e21

namespace {

/* libm through a pointer the compiler cannot see through: pow as the reference calls it */
double (*volatile libm_pow)(double, double) = pow;

constexpr int LT = 256;
constexpr int LENS_CCHUNK = 8;         /* cuts one projection launch accumulates in registers: the mesh is read once per normal for <= 8 cuts */
constexpr int LENS_WRAP_CAP = 1 << 20; /* guard of the periodic while loops (the reference loops for ever on a position 2^20 boxes away) */
constexpr long long LENS_MAX_PLANES = 65535; /* the density kernel's grid y */

/* the normal-axis bin of one (cut, normal): bins[0] and bins[1] - bins[0] of linspace(center - th / 2, center + th / 2, 2) */
struct LensCut {
    double b0, w;
};
/* the particle pass' constants */
struct LensGeo {
    double L, off[3];
    double wP;       /* bins[R] - bins[0] of the plane axes' linspace(0, L, R + 1) */
    int R, nu, ncuts, excl2;
    int normal[3];   /* the distinct normals, in order of first request */
};

/* grid3d_ngb: into (0, L] */
__device__ __forceinline__ double wrap_oc(double x, double L)
{
#pragma clang fp contract(off)
    for(int k = 0; x > L && k < LENS_WRAP_CAP; k++)
        x -= L;
    for(int k = 0; x <= 0 && k < LENS_WRAP_CAP; k++)
        x += L;
    return x;
}

/* find_bin (lenstools.cpp:68-95): -1 when dropped */
__device__ __forceinline__ int find_bin(double value, double b0, double width, int res, double L)
{
#pragma clang fp contract(off)
    if(width <= 0)
        return -1;
    double rel = value - b0;
    for(int k = 0; rel < 0 && k < LENS_WRAP_CAP; k++)
        rel += L;
    for(int k = 0; rel >= L && k < LENS_WRAP_CAP; k++)
        rel -= L;
    if(rel >= width)
        return -1;
    const double iflt = rel / width * res;
    const double f = floor(iflt);
    if(!(f >= 0 && f < res))
        return -1;
    return (int) f;
}

/* the particle pass: activity (lenstools_particle_is_active: not Swallowed, not Type 2 under exclude_type2), the block's active count,
 * and (counts != NULL) one u32 add per accepting (cut, normal) into counts[(cut * nu + u) * R^2 + row * R + col] */
__global__ __launch_bounds__(LT) void lens_bin_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                      const LensGeo g, const LensCut *__restrict__ cuts, uint32_t *__restrict__ counts,
                                                      unsigned long long *__restrict__ nactive)
{
#pragma clang fp contract(off)
    const long long i = (long long) blockIdx.x * LT + threadIdx.x;
    bool act = false;
    if(i < n) {
        const unsigned f = pflags[i];
        act = !(f & 2u) && !(g.excl2 && (f >> 4) == 2);
    }
    const int c = __syncthreads_count(act);
    if(threadIdx.x == 0 && c)
        atomicAdd(nactive, (unsigned long long) c);
    if(!act || !counts)
        return;
    const double4 p = posm[i];
    const double x = wrap_oc(p.x - g.off[0], g.L), y = wrap_oc(p.y - g.off[1], g.L), z = wrap_oc(p.z - g.off[2], g.L);
    /* the plane axes' bins: bins[0] = 0 + 0 * step = 0 (left_corner 0) */
    const int bx = find_bin(x, 0.0, g.wP, g.R, g.L), by = find_bin(y, 0.0, g.wP, g.R, g.L), bz = find_bin(z, 0.0, g.wP, g.R, g.L);
    const size_t plane = (size_t) g.R * g.R;
    for(int u = 0; u < g.nu; u++) {
        const int nrm = g.normal[u];
        /* projectDensity's layout: normal 0 -> [y][z], 1 -> [x][z], 2 -> [x][y] */
        const int a = nrm == 0 ? by : bx, b = nrm == 2 ? by : bz;
        if(a < 0 || b < 0)
            continue;
        const double v = nrm == 0 ? x : (nrm == 1 ? y : z);
        const size_t pix = (size_t) a * g.R + b;
        for(int k = 0; k < g.ncuts; k++) {
            const LensCut ct = cuts[k * g.nu + u];
            if(find_bin(v, ct.b0, ct.w, 1, g.L) < 0)
                continue;
            atomicAdd(&counts[(size_t) (k * g.nu + u) * plane + pix], 1u);
        }
    }
}

/* counts -> density (count * the plane's factor) and each plane's count sum; grid (blocks, planes) */
__global__ __launch_bounds__(LT) void lens_density_kernel(const uint32_t *__restrict__ counts, size_t plane, const double *__restrict__ dnf,
                                                          double *__restrict__ dens, unsigned long long *__restrict__ psum)
{
    __shared__ unsigned long long s;
    if(threadIdx.x == 0)
        s = 0;
    __syncthreads();
    const size_t p = blockIdx.y;
    const double f = dnf[p];
    unsigned long long t = 0;
    for(size_t k = (size_t) blockIdx.x * LT + threadIdx.x; k < plane; k += (size_t) gridDim.x * LT) {
        const uint32_t c = counts[p * plane + k];
        t += c;
        dens[p * plane + k] = (double) c * f;
    }
    if(t)
        atomicAdd(&s, t);
    __syncthreads();
    if(threadIdx.x == 0 && s)
        atomicAdd(&psum[p], s);
}

/* one plane's solve constants: b0 b1 / chi^2 of the Poisson factor, the final scale (cosmo_normalization density_normalization / R^2),
 * and whether the plane is empty (then every mode becomes 0) */
struct LensSolve {
    double pref, scale;
    int32_t empty, pad_;
};

/* calculate_lensing_potential's spectral part on the [planes][R][R/2 + 1] half spectra: DC to zero, factor * exp(.), the final scale */
__global__ __launch_bounds__(LT) void lens_filter_kernel(double2 *spec, int R, long long nplanes, const LensSolve *__restrict__ sp, double g2)
{
#pragma clang fp contract(off)
    const int Rh = R / 2 + 1;
    const long long per = (long long) R * Rh, total = per * nplanes;
    for(long long e = (long long) blockIdx.x * LT + threadIdx.x; e < total; e += (long long) gridDim.x * LT) {
        const long long p = e / per;
        const long long r = e - p * per;
        const int i = (int) (r / Rh), j = (int) (r - (long long) i * Rh);
        const LensSolve s = sp[p];
        if(s.empty || (i == 0 && j == 0)) {
            spec[e] = make_double2(0.0, 0.0);
            continue;
        }
        double lx = i < R / 2 ? i : -(R - i);
        lx /= R;
        double ly = j;
        ly /= R;
        const double l2 = lx * lx + ly * ly;
        const double factor = -2.0 * s.pref / (l2 * 4 * M_PI * M_PI);
        const double m = factor * exp(-0.5 * g2 * l2);
        const double2 v = spec[e];
        spec[e] = make_double2(v.x * m * s.scale, v.y * m * s.scale);
    }
}

/* cutPlanePMNeutrinoCorrection's projection along x (normal 0: [y][z]) or y (normal 1: [z][x], the reference's transpose): one thread
 * per output pixel, the normal-axis cells in ascending order; w: overlap per global normal-axis cell and cut [N][ncuts] */
template <int NORMAL>
__global__ __launch_bounds__(LT) void lens_project_xy_kernel(const double *__restrict__ mesh, int N, int x0, int nx, const double *__restrict__ w,
                                                             int ncuts, int c0, int nc, double inv_fft_norm, double mean_mass_cell, double th,
                                                             int nu, int u, double *proj)
{
#pragma clang fp contract(off)
    const long long M = NORMAL == 0 ? (long long) N * N : (long long) nx * N;
    const long long t = (long long) blockIdx.x * LT + threadIdx.x;
    if(t >= M)
        return;
    const long long NN = (long long) N * N;
    long long base, stride, out;
    int K, k0;
    if(NORMAL == 0) { /* pixel (y, z); cells x */
        base = t;
        stride = NN;
        K = nx;
        k0 = x0;
        out = t;
    } else {          /* pixel (x, z); cells y; output [z][x] */
        const long long ix = t / N, z = t - ix * N;
        base = ix * NN + z;
        stride = N;
        K = N;
        k0 = 0;
        out = z * N + (x0 + ix);
    }
    double acc[LENS_CCHUNK];
#pragma unroll
    for(int c = 0; c < LENS_CCHUNK; c++)
        acc[c] = 0.0;
    for(int k = 0; k < K; k++) {
        const double delta = mesh[base + (long long) k * stride] * inv_fft_norm / mean_mass_cell;
        const double *wk = w + (size_t) (k0 + k) * ncuts + c0;
#pragma unroll
        for(int c = 0; c < LENS_CCHUNK; c++)
            if(c < nc && wk[c] > 0)
                acc[c] += delta * wk[c] / th;
    }
#pragma unroll
    for(int c = 0; c < LENS_CCHUNK; c++)
        if(c < nc)
            proj[((size_t) (c0 + c) * nu + u) * NN + out] = acc[c];
}

/* the projection along z (normal 2: [x][y]): one wave per (x, y) row, lanes over z, a fixed butterfly across the wave */
__global__ __launch_bounds__(LT) void lens_project_z_kernel(const double *__restrict__ mesh, int N, int x0, int nx, const double *__restrict__ w,
                                                            int ncuts, int c0, int nc, double inv_fft_norm, double mean_mass_cell, double th,
                                                            int nu, int u, double *proj)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long row = ((long long) blockIdx.x * LT + threadIdx.x) >> 6;
    if(row >= (long long) nx * N) /* wave-uniform */
        return;
    const double *m = mesh + row * N;
    double acc[LENS_CCHUNK];
#pragma unroll
    for(int c = 0; c < LENS_CCHUNK; c++)
        acc[c] = 0.0;
    for(int z = lane; z < N; z += 64) {
        const double delta = m[z] * inv_fft_norm / mean_mass_cell;
        const double *wk = w + (size_t) z * ncuts + c0;
#pragma unroll
        for(int c = 0; c < LENS_CCHUNK; c++)
            if(c < nc && wk[c] > 0)
                acc[c] += delta * wk[c] / th;
    }
#pragma unroll
    for(int c = 0; c < LENS_CCHUNK; c++)
        for(int o = 32; o > 0; o >>= 1)
            acc[c] += __shfl_xor(acc[c], o, 64);
    if(lane == 0) {
        const long long ix = row / N, y = row - ix * N;
        const size_t NN = (size_t) N * N;
#pragma unroll
        for(int c = 0; c < LENS_CCHUNK; c++)
            if(c < nc)
                proj[((size_t) (c0 + c) * nu + u) * NN + (size_t) (x0 + ix) * N + y] = acc[c];
    }
}

/* plane_add_periodic_bilinear: dst[p] (R^2) += src[p] (N^2) interpolated, every plane p */
__global__ __launch_bounds__(LT) void lens_bilinear_kernel(double *dst, int R, const double *__restrict__ src, int N, long long nplanes)
{
#pragma clang fp contract(off)
    const long long per = (long long) R * R, total = per * nplanes;
    for(long long e = (long long) blockIdx.x * LT + threadIdx.x; e < total; e += (long long) gridDim.x * LT) {
        const long long p = e / per;
        const long long r = e - p * per;
        const int i = (int) (r / R), j = (int) (r - (long long) i * R);
        const double x = ((i + 0.5) * N / R) - 0.5;
        int i0 = (int) floor(x);
        const double tx = x - i0;
        while(i0 < 0)
            i0 += N;
        while(i0 >= N)
            i0 -= N;
        const int i1 = (i0 + 1) % N;
        const double y = ((j + 0.5) * N / R) - 0.5;
        int j0 = (int) floor(y);
        const double ty = y - j0;
        while(j0 < 0)
            j0 += N;
        while(j0 >= N)
            j0 -= N;
        const int j1 = (j0 + 1) % N;
        const double *s = src + (size_t) p * N * N;
        const double v00 = s[(size_t) i0 * N + j0], v10 = s[(size_t) i1 * N + j0];
        const double v01 = s[(size_t) i0 * N + j1], v11 = s[(size_t) i1 * N + j1];
        dst[e] += (1 - tx) * (1 - ty) * v00 + tx * (1 - ty) * v10 + (1 - tx) * ty * v01 + tx * ty * v11;
    }
}

/* the particles' positions and flag bytes (stage_part_view); the binning reads IsGarbage and Swallowed, so a staged view needs the flag word */
int lens_particles(shq_context *ctx, CallScope &sc, const shq_part_view *parts, const double4 **d_posm, const uint8_t **d_flags)
{
    SHQ_CHECK(parts_resident(ctx, parts) || (parts->off_pos != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD && parts->off_flags != SHQ_NOFIELD),
              SHQ_ERR_INVALID, "lens: the particle view needs Pos, Type and the flag word");
    return stage_part_view(ctx, sc, parts, false, d_posm, d_flags);
}

/* linspace (lenstools.cpp:39-44), entry i */
double linspace_at(double start, double stop, int num, int i)
{
#pragma clang fp contract(off)
    const double step = (stop - start) / (num - 1);
    return start + i * step;
}

/* plane_periodic_slab_overlap with plane_interval_overlap (plane.cpp:355-381) */
double slab_overlap(double cell_start, double cellsize, double center, double thickness, double L)
{
#pragma clang fp contract(off)
    if(thickness >= L)
        return cellsize;
    double c = center;
    while(c < 0)
        c += L;
    while(c >= L)
        c -= L;
    const double slab_start = c - 0.5 * thickness;
    const double slab_end = slab_start + thickness;
    const double cell_end = cell_start + cellsize;
    double overlap = 0.0;
    for(int shift = -1; shift <= 1; shift++) {
        const double offset = shift * L;
        const double b0 = slab_start + offset, b1 = slab_end + offset;
        const double lo = cell_start > b0 ? cell_start : b0;
        const double hi = cell_end < b1 ? cell_end : b1;
        overlap += hi > lo ? hi - lo : 0.0;
    }
    return overlap;
}

/* the effective thickness and cut count of write_plane's defaults (plane.cpp:519-530) */
int lens_cuts(const shq_lens_params *p, double *th, int64_t *ncuts)
{
    SHQ_CHECK(isfinite(p->BoxSize) && p->BoxSize > 0 && !isnan(p->Thickness), SHQ_ERR_INVALID, "lens: BoxSize must be finite and > 0");
    *th = p->Thickness <= 0.0 ? p->BoxSize : p->Thickness;
    SHQ_CHECK(isfinite(*th), SHQ_ERR_INVALID, "lens: Thickness must be finite");
    SHQ_CHECK(p->ncuts >= 0, SHQ_ERR_INVALID, "lens: ncuts %d < 0", p->ncuts);
    if(p->ncuts > 0) {
        *ncuts = p->ncuts;
        return SHQ_OK;
    }
    const double d = p->BoxSize / *th;
    SHQ_CHECK(d < (double) LENS_MAX_PLANES, SHQ_ERR_INVALID, "lens: the default cut list would hold %g cuts", d);
    *ncuts = (int64_t) (size_t) d;
    return SHQ_OK;
}

/* a grid-stride launch: no more than cap blocks */
inline unsigned nblk_cap(long long n, long long cap) { return (unsigned) std::min<long long>(nblk(n, LT), cap); }

/* calculate_lensing_potential on nplanes real planes [nplanes][R][R] at dens, through the half spectra at spec, into out */
int lens_solve(CallScope &sc, int R, int nplanes, double *dens, double2 *spec, double *out, const LensSolve *d_sp)
{
    hipfftHandle f, b;
    int dims[2] = {R, R};
    SHQ_TRY(sc.plan_many(2, dims, HIPFFT_D2Z, nplanes, &f));
    SHQ_TRY(sc.plan_many(2, dims, HIPFFT_Z2D, nplanes, &b));
    hipfftResult r = hipfftExecD2Z(f, (hipfftDoubleReal *) dens, (hipfftDoubleComplex *) spec);
    SHQ_CHECK(r == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "lens: hipfftExecD2Z failed: %d", (int) r);
    const long long nspec = (long long) R * (R / 2 + 1) * nplanes;
    const double g2 = (2.0 * M_PI * 1.0) * (2.0 * M_PI * 1.0); /* (2 pi smooth)^2, smooth = 1 */
    lens_filter_kernel<<<dim3(nblk_cap(nspec, 4096)), dim3(LT), 0, sc.ctx->stream>>>(spec, R, nplanes, d_sp, g2);
    SHQ_HIP(hipGetLastError());
    r = hipfftExecZ2D(b, (hipfftDoubleComplex *) spec, (hipfftDoubleReal *) out);
    SHQ_CHECK(r == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "lens: hipfftExecZ2D failed: %d", (int) r);
    return SHQ_OK;
}

} // namespace

/* ---- C-ABI ------------------------------------------------------------------------------ */

extern "C" int shq_lens_num_cuts(const shq_lens_params *p, int32_t *ncuts)
{
    SHQ_CHECK(p && ncuts, SHQ_ERR_INVALID, "lens: null argument");
    double th = 0;
    int64_t nc = 0;
    SHQ_TRY(lens_cuts(p, &th, &nc));
    *ncuts = (int32_t) nc;
    return SHQ_OK;
}

extern "C" int shq_lens_phase_ms(shq_context *ctx, double ms[4])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 4; i++)
        ms[i] = ctx->lens_ms[i];
    return SHQ_OK;
}

extern "C" int shq_lens_count_active(shq_context *ctx, const shq_part_view *parts, int exclude_type2, int64_t *count)
{
    SHQ_CHECK(ctx && parts && count, SHQ_ERR_INVALID, "lens: null argument");
    SHQ_HIP(hipSetDevice(ctx->device));
    CallScope sc(ctx, "lens");
    const double4 *d_posm;
    const uint8_t *d_flags;
    SHQ_TRY(lens_particles(ctx, sc, parts, &d_posm, &d_flags));
    const long long n = parts->numpart;
    unsigned long long *d_n;
    SHQ_TRY(sc.alloc(&d_n, 1));
    SHQ_HIP(hipMemsetAsync(d_n, 0, sizeof(unsigned long long), ctx->stream));
    LensGeo g;
    memset(&g, 0, sizeof(g));
    g.excl2 = exclude_type2 != 0;
    if(n > 0)
        lens_bin_kernel<<<dim3(nblk(n)), dim3(LT), 0, ctx->stream>>>(n, d_posm, d_flags, g, nullptr, nullptr, d_n);
    SHQ_HIP(hipGetLastError());
    unsigned long long h = 0;
    SHQ_HIP(hipMemcpyAsync(&h, d_n, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    *count = (int64_t) h;
    return SHQ_OK;
}

extern "C" int shq_lens_planes(shq_context *ctx, const shq_lens_params *p, const shq_lens_cosmo *c, const shq_part_view *parts,
                               const shq_lens_numesh *nu, double *planes, int64_t *num_particles_plane, uint32_t *counts)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && p && c && parts && planes && num_particles_plane, SHQ_ERR_INVALID, "lens: null argument");
    /* ---- every check before anything is written (the reference ends the run in each of these cases) */
    double th = 0;
    int64_t ncuts = 0;
    SHQ_TRY(lens_cuts(p, &th, &ncuts));
    const int R = p->Resolution;
    SHQ_CHECK(R >= 2 && R <= 46340, SHQ_ERR_INVALID, "lens: PlaneResolution %d must be in [2, 46340]", R);
    SHQ_CHECK(p->nnormals >= 1 && p->Normals, SHQ_ERR_INVALID, "lens: no normals");
    SHQ_CHECK(p->ncuts == 0 || p->CutPoints, SHQ_ERR_INVALID, "lens: ncuts > 0 without CutPoints");
    for(int j = 0; j < p->nnormals; j++)
        SHQ_CHECK(p->Normals[j] >= 0 && p->Normals[j] <= 2, SHQ_ERR_INVALID, "Requesting a normal direction beyond 0, 1 and 2: %d", p->Normals[j]);
    for(int k = 0; k < p->ncuts; k++)
        SHQ_CHECK(isfinite(p->CutPoints[k]), SHQ_ERR_INVALID, "lens: non-finite cut point");
    SHQ_CHECK(isfinite(p->CurrentParticleOffset[0]) && isfinite(p->CurrentParticleOffset[1]) && isfinite(p->CurrentParticleOffset[2]),
              SHQ_ERR_INVALID, "lens: non-finite particle offset");
    SHQ_CHECK(c->num_particles_tot > 0, SHQ_ERR_INVALID, "Cannot build a potential plane from zero active particle count.");
    SHQ_CHECK(c->omega_source > 0, SHQ_ERR_INVALID, "Non-positive particle matter density for potential plane: OmegaSource = %g", c->omega_source);
    SHQ_CHECK(c->atime > 0 && c->HubbleParam > 0 && isfinite(c->comoving_distance), SHQ_ERR_INVALID, "lens: atime and HubbleParam must be > 0");
    if(nu) {
        SHQ_CHECK(nu->Nmesh >= 2 && nu->Nmesh <= 4096, SHQ_ERR_INVALID, "lens: correction Nmesh %d must be in [2, 4096]", nu->Nmesh);
        SHQ_CHECK(nu->x0 >= 0 && nu->nx >= 1 && (int64_t) nu->x0 + nu->nx <= nu->Nmesh, SHQ_ERR_INVALID,
                  "lens: correction slab x0 %d, nx %d outside [0, %d)", nu->x0, nu->nx, nu->Nmesh);
        SHQ_CHECK(nu->real, SHQ_ERR_INVALID, "lens: correction without a mesh");
    }
    const long long n = parts->numpart;
    SHQ_CHECK(n >= 0 && n < (1ll << 32), SHQ_ERR_INVALID, "lens: %lld particles on one rank (< 2^32)", n);
    /* the distinct normals; planes on the device are [cut][distinct normal] */
    int unorm[3] = {0, 0, 0}, nuq = 0;
    std::vector<int> map((size_t) p->nnormals);
    for(int j = 0; j < p->nnormals; j++) {
        int u = 0;
        while(u < nuq && unorm[u] != p->Normals[j])
            u++;
        if(u == nuq)
            unorm[nuq++] = p->Normals[j];
        map[j] = u;
    }
    const long long P = ncuts * nuq;
    SHQ_CHECK(P <= LENS_MAX_PLANES, SHQ_ERR_INVALID, "lens: %lld planes (%lld at most)", P, LENS_MAX_PLANES);
    SHQ_HIP(hipSetDevice(ctx->device));
    for(int i = 0; i < 4; i++)
        ctx->lens_ms[i] = 0;
    if(P == 0)
        return SHQ_OK;

    const double L = p->BoxSize;
    std::vector<double> cutv((size_t) ncuts);
    for(int64_t k = 0; k < ncuts; k++)
        cutv[k] = p->ncuts > 0 ? p->CutPoints[k] : (.5 + k) * th;
    hipStream_t s = ctx->stream;
    CallScope sc(ctx, "lens");
    SHQ_TRY(sc.mark(s));

    /* ---- the particle pass */
    const double4 *d_posm;
    const uint8_t *d_flags;
    SHQ_TRY(lens_particles(ctx, sc, parts, &d_posm, &d_flags));
    LensGeo g;
    memset(&g, 0, sizeof(g));
    g.L = L;
    for(int d = 0; d < 3; d++)
        g.off[d] = p->CurrentParticleOffset[d];
    g.wP = linspace_at(0, 0 + L, R + 1, R) - linspace_at(0, 0 + L, R + 1, 0);
    g.R = R;
    g.nu = nuq;
    g.ncuts = (int) ncuts;
    g.excl2 = p->exclude_type2 != 0;
    for(int u = 0; u < nuq; u++)
        g.normal[u] = unorm[u];
    std::vector<LensCut> hc((size_t) P);
    for(int64_t k = 0; k < ncuts; k++)
        for(int u = 0; u < nuq; u++) {
            const double start = cutv[k] - th / 2, stop = cutv[k] + th / 2;
            hc[(size_t) (k * nuq + u)] = {linspace_at(start, stop, 2, 0), linspace_at(start, stop, 2, 1) - linspace_at(start, stop, 2, 0)};
        }
    const size_t plane = (size_t) R * R;
    LensCut *d_cuts;
    uint32_t *d_counts;
    unsigned long long *d_nact, *d_psum;
    SHQ_TRY(sc.alloc(&d_cuts, (size_t) P));
    SHQ_TRY(sc.alloc(&d_counts, (size_t) P * plane));
    SHQ_TRY(sc.alloc(&d_nact, 1));
    SHQ_TRY(sc.alloc(&d_psum, (size_t) P));
    SHQ_HIP(hipMemcpyAsync(d_cuts, hc.data(), sizeof(LensCut) * P, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * P * plane, s));
    SHQ_HIP(hipMemsetAsync(d_nact, 0, sizeof(unsigned long long), s));
    SHQ_HIP(hipMemsetAsync(d_psum, 0, sizeof(unsigned long long) * P, s));
    if(n > 0)
        lens_bin_kernel<<<dim3(nblk(n)), dim3(LT), 0, s>>>(n, d_posm, d_flags, g, d_cuts, d_counts, d_nact);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(sc.mark(s)); /* ev[1]: the particle pass */

    /* ---- counts -> density and the plane sums; the 2-D solves of all particle planes in one batch */
    const double H0 = 100 * c->HubbleParam * 3.2407793e-20;
    const double cosmo_normalization = 1.5 * libm_pow(H0, 2) * c->omega_source / libm_pow(LENS_LIGHTCGS, 2);
    const double density_normalization = th * c->comoving_distance * libm_pow(LENS_CM_PER_KPC / c->HubbleParam, 2) / c->atime;
    const double chi = c->comoving_distance;
    std::vector<double> dnf((size_t) P);
    for(int64_t k = 0; k < ncuts; k++)
        for(int u = 0; u < nuq; u++) {
            double b[3] = {L / R, L / R, L / R};
            b[unorm[u]] = th / 1;
            dnf[(size_t) (k * nuq + u)] = 1. / c->num_particles_tot * (libm_pow(L, 3) / (b[0] * b[1] * b[2]));
        }
    double *d_dnf, *d_dens, *d_out;
    double2 *d_spec;
    LensSolve *d_sp;
    SHQ_TRY(sc.alloc(&d_dnf, (size_t) P));
    SHQ_TRY(sc.alloc(&d_dens, (size_t) P * plane));
    SHQ_TRY(sc.alloc(&d_out, (size_t) P * plane));
    SHQ_TRY(sc.alloc(&d_spec, (size_t) P * R * (R / 2 + 1)));
    SHQ_TRY(sc.alloc(&d_sp, (size_t) P));
    SHQ_HIP(hipMemcpyAsync(d_dnf, dnf.data(), sizeof(double) * P, hipMemcpyHostToDevice, s));
    lens_density_kernel<<<dim3(nblk_cap((long long) plane, 256), (unsigned) P), dim3(LT), 0, s>>>(d_counts, plane, d_dnf, d_dens, d_psum);
    SHQ_HIP(hipGetLastError());
    std::vector<unsigned long long> psum((size_t) P);
    SHQ_HIP(hipMemcpyAsync(psum.data(), d_psum, sizeof(unsigned long long) * P, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    std::vector<LensSolve> sp((size_t) P);
    for(long long q = 0; q < P; q++)
        sp[q] = {(L / R) * (L / R) / (chi * chi), cosmo_normalization * density_normalization / (double) (R * R), psum[q] == 0, 0};
    SHQ_HIP(hipMemcpyAsync(d_sp, sp.data(), sizeof(LensSolve) * P, hipMemcpyHostToDevice, s));
    SHQ_TRY(lens_solve(sc, R, (int) P, d_dens, d_spec, d_out, d_sp));
    SHQ_TRY(sc.mark(s)); /* ev[2]: the particle planes solved */

    /* ---- the PM neutrino correction: project per distinct normal, solve at Nmesh, add bilinearly */
    if(nu) {
        const int N = nu->Nmesh;
        const size_t NN = (size_t) N * N, slab = (size_t) nu->nx * NN;
        const double cellsize = L / N;
        std::vector<double> w((size_t) N * ncuts); /* [normal-axis cell][cut]: the same for every normal */
        for(int k = 0; k < N; k++)
            for(int64_t q = 0; q < ncuts; q++)
                w[(size_t) k * ncuts + q] = slab_overlap(k * cellsize, cellsize, cutv[q], th, L);
        double *d_mesh, *d_w, *d_proj, *d_corr;
        double2 *d_cspec;
        LensSolve *d_csp;
        SHQ_TRY(sc.alloc(&d_mesh, slab));
        SHQ_TRY(sc.alloc(&d_w, w.size()));
        SHQ_TRY(sc.alloc(&d_proj, (size_t) P * NN));
        SHQ_TRY(sc.alloc(&d_corr, (size_t) P * NN));
        SHQ_TRY(sc.alloc(&d_cspec, (size_t) P * N * (N / 2 + 1)));
        SHQ_TRY(sc.alloc(&d_csp, (size_t) P));
        SHQ_HIP(hipMemcpyAsync(d_mesh, nu->real, sizeof(double) * slab, hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemcpyAsync(d_w, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemsetAsync(d_proj, 0, sizeof(double) * P * NN, s));
        const int nct = (int) ncuts;
        for(int u = 0; u < nuq; u++)
            for(int c0 = 0; c0 < nct; c0 += LENS_CCHUNK) {
                const int nc = std::min(LENS_CCHUNK, nct - c0);
                if(unorm[u] == 0)
                    lens_project_xy_kernel<0><<<dim3(nblk((long long) NN)), dim3(LT), 0, s>>>(d_mesh, N, nu->x0, nu->nx, d_w, nct, c0, nc,
                                                                                           nu->inv_fft_norm, nu->mean_mass_cell, th, nuq, u, d_proj);
                else if(unorm[u] == 1)
                    lens_project_xy_kernel<1><<<dim3(nblk((long long) nu->nx * N)), dim3(LT), 0, s>>>(d_mesh, N, nu->x0, nu->nx, d_w, nct, c0, nc,
                                                                                                   nu->inv_fft_norm, nu->mean_mass_cell, th, nuq, u, d_proj);
                else
                    lens_project_z_kernel<<<dim3(nblk((long long) nu->nx * N * 64)), dim3(LT), 0, s>>>(d_mesh, N, nu->x0, nu->nx, d_w, nct, c0, nc,
                                                                                                    nu->inv_fft_norm, nu->mean_mass_cell, th, nuq, u, d_proj);
                SHQ_HIP(hipGetLastError());
            }
        std::vector<LensSolve> csp((size_t) P);
        for(long long q = 0; q < P; q++)
            csp[q] = {cellsize * cellsize / (chi * chi), cosmo_normalization * density_normalization / (double) (N * N), 0, 0};
        SHQ_HIP(hipMemcpyAsync(d_csp, csp.data(), sizeof(LensSolve) * P, hipMemcpyHostToDevice, s));
        SHQ_TRY(lens_solve(sc, N, (int) P, d_proj, d_cspec, d_corr, d_csp));
        lens_bilinear_kernel<<<dim3(nblk_cap((long long) P * plane, 4096)), dim3(LT), 0, s>>>(d_out, R, d_corr, N, P);
        SHQ_HIP(hipGetLastError());
    }
    SHQ_TRY(sc.mark(s)); /* ev[3]: the correction added */

    /* ---- out: [cut][requested normal]; repeated normals share their plane */
    for(int64_t k = 0; k < ncuts; k++)
        for(int j = 0; j < p->nnormals; j++) {
            const size_t q = (size_t) (k * nuq + map[j]), o = (size_t) (k * p->nnormals + j);
            SHQ_HIP(hipMemcpyAsync(planes + o * plane, d_out + q * plane, sizeof(double) * plane, hipMemcpyDeviceToHost, s));
            if(counts)
                SHQ_HIP(hipMemcpyAsync(counts + o * plane, d_counts + q * plane, sizeof(uint32_t) * plane, hipMemcpyDeviceToHost, s));
            num_particles_plane[o] = (int64_t) psum[q];
        }
    SHQ_TRY(sc.mark(s)); /* ev[4]: downloaded */
    SHQ_HIP(hipStreamSynchronize(s));
    ctx->lens_ms[0] = sc.ms(0, 1);
    ctx->lens_ms[1] = sc.ms(1, 2);
    ctx->lens_ms[2] = sc.ms(2, 3);
    ctx->lens_ms[3] = sc.ms(0, 4);
    return SHQ_OK;
}
