/* mesh_common.hpp — the plumbing the one-call mesh operators share (glass, zeldovich, uvbg, lens; the convert kernel also serves pm.hip):
 * the mesh-size check, the two routes of a 3-D transform, the modes of a half spectrum, and a particle view staged on the device. */
#pragma once
#include "call_scope.hpp"
#include "cic.hpp"
#include <math.h>

inline int mesh_check_size(int N, const char *who)
{
    SHQ_CHECK(N >= 4 && N % 2 == 0 && N <= 2048, SHQ_ERR_INVALID, "%s: Nmesh must be even and in [4, 2048] (got %d)", who, N);
    return SHQ_OK;
}

/* a mesh deposited in 64-bit fixed point as doubles, in place (grid-stride: any launch shape) */
static __global__ void mesh_convert_i64_kernel(double *mesh, size_t n, double inv_scale)
{
    const long long *im = reinterpret_cast<const long long *>(mesh);
    const size_t stride = (size_t) gridDim.x * blockDim.x;
    for(size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        mesh[i] = (double) im[i] * inv_scale;
}

/* ---- the in-place r2c / c2r of a mesh [N][N][zp]: the five-pass pipeline of fft3d.hip where it has the size, hipFFT otherwise */
struct Fft3dRoute {
    int N;
    bool bespoke;
    int zp;        /* doubles per z row */
    size_t padded; /* N N zp */
    hipfftHandle fwd = 0, inv = 0; /* the hipFFT route's plans (route_plans), owned by the call's scope */
};

inline Fft3dRoute fft3d_route(int N)
{
    Fft3dRoute r;
    r.N = N;
    r.bespoke = shq_fft3d_supported(N) && N % 8 == 0;
    r.zp = r.bespoke ? shq_fft3d_pitch(N) : N + 2;
    r.padded = (size_t) N * N * r.zp;
    return r;
}

/* the plans the hipFFT route needs, made once per call */
inline int route_plans(CallScope &sc, Fft3dRoute &r, bool forward, bool inverse)
{
    if(r.bespoke)
        return SHQ_OK;
    if(forward)
        SHQ_TRY(sc.plan3d(r.N, HIPFFT_D2Z, &r.fwd));
    if(inverse)
        SHQ_TRY(sc.plan3d(r.N, HIPFFT_Z2D, &r.inv));
    return SHQ_OK;
}

/* hipFFT's half of the two transforms, for a caller whose bespoke side is its own (uvbg) */
inline int route_hipfft_forward(CallScope &sc, const Fft3dRoute &r, double *d_mesh)
{
    const hipfftResult rc = hipfftExecD2Z(r.fwd, (hipfftDoubleReal *) d_mesh, (hipfftDoubleComplex *) d_mesh);
    SHQ_CHECK(rc == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "%s: hipfftExecD2Z failed: %d", sc.who, (int) rc);
    return SHQ_OK;
}

inline int route_hipfft_inverse(CallScope &sc, const Fft3dRoute &r, double *d_mesh)
{
    const hipfftResult rc = hipfftExecZ2D(r.inv, (hipfftDoubleComplex *) d_mesh, (hipfftDoubleReal *) d_mesh);
    SHQ_CHECK(rc == HIPFFT_SUCCESS, SHQ_ERR_DEVICE, "%s: hipfftExecZ2D failed: %d", sc.who, (int) rc);
    return SHQ_OK;
}

/* the unscaled r2c; from_i64: the mesh holds the fixed-point deposit, worth inv_scale per unit */
inline int route_forward(shq_context *ctx, CallScope &sc, const Fft3dRoute &r, double *d_mesh, bool from_i64, double inv_scale)
{
    if(r.bespoke)
        return shq_fft3d_run(ctx, d_mesh, r.N, r.zp, SHQ_FFT_FORWARD, from_i64, inv_scale, nullptr, 0, 0);
    if(from_i64) {
        mesh_convert_i64_kernel<<<dim3(nblk((long long) r.padded)), dim3(256), 0, ctx->stream>>>(d_mesh, r.padded, inv_scale);
        SHQ_HIP(hipGetLastError());
    }
    return route_hipfft_forward(sc, r, d_mesh);
}

/* the unscaled c2r */
inline int route_inverse(shq_context *ctx, CallScope &sc, const Fft3dRoute &r, double *d_mesh)
{
    if(r.bespoke)
        return shq_fft3d_run(ctx, d_mesh, r.N, r.zp, SHQ_FFT_INVERSE, false, 1.0, nullptr, 0, 0);
    return route_hipfft_inverse(sc, r, d_mesh);
}

/* ---- mode ip of a half spectrum [x][y][z'], z' < N / 2 + 1: the signed wave numbers, k2, and the row x N + y */
struct HalfMode {
    int x, y, z, kx, ky;
    long long k2;
    size_t row;
};

__device__ __forceinline__ HalfMode half_mode(size_t ip, int N)
{
    const int Nc = N / 2 + 1;
    HalfMode m;
    m.z = (int) (ip % Nc);
    m.row = ip / Nc;
    m.y = (int) (m.row % N);
    m.x = (int) (m.row / N);
    m.kx = m.x <= N / 2 ? m.x : m.x - N;
    m.ky = m.y <= N / 2 ? m.y : m.y - N;
    m.k2 = (long long) m.kx * m.kx + (long long) m.ky * m.ky + (long long) m.z * m.z;
    return m;
}

/* ---- particles */

/* the context holds these very particles, with their types, and the caller vouches that the copy is current */
inline bool parts_resident(const shq_context *ctx, const shq_part_view *parts)
{
    return (ctx->inputs_current & SHQ_CURRENT_PARTICLES) && ctx->have_parts && ctx->have_types && ctx->cur_parts == parts->base &&
           ctx->cur_parts_n == parts->numpart && ctx->numpart == parts->numpart;
}

/* The particles' (Pos, Mass) and flag bytes on the device: the resident set, or the view packed into buffers of the call's own.
 * The byte has the context's layout (shq_particles_upload): Type in bits 4-7, and IsGarbage, Swallowed, HeIIIionized in bits 0-2
 * where the view has the flag word.  A caller that reads only the type (uvbg, >> 4) does not see the low bits.  Without want_mass
 * the fourth component is 0 and the view needs no Mass. */
inline int stage_part_view(shq_context *ctx, CallScope &sc, const shq_part_view *parts, bool want_mass, const double4 **d_posm,
                           const uint8_t **d_flags)
{
    const long long n = parts->numpart;
    SHQ_CHECK(n >= 0 && n < (1ll << 32) && (n == 0 || parts->base), SHQ_ERR_INVALID, "%s: bad particle view (numpart %lld; < 2^32 per rank)", sc.who, n);
    if(parts_resident(ctx, parts)) {
        *d_posm = ctx->posm.ptr;
        *d_flags = ctx->pflags.ptr;
        return SHQ_OK;
    }
    SHQ_CHECK(parts->off_pos != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD && (!want_mass || parts->off_mass != SHQ_NOFIELD), SHQ_ERR_INVALID,
              "%s: the particle view needs Pos, Type%s", sc.who, want_mass ? " and Mass" : "");
    double4 *pm4;
    uint8_t *fl;
    SHQ_TRY(sc.alloc(&pm4, (size_t) n));
    SHQ_TRY(sc.alloc(&fl, (size_t) n));
    std::vector<double4> h4((size_t) n);
    std::vector<uint8_t> hf((size_t) n);
    const char *b = (const char *) parts->base;
    const bool low = parts->off_flags != SHQ_NOFIELD;
    bool finite = true;
    for(long long i = 0; i < n; i++) {
        const char *r = b + (size_t) i * parts->elsize;
        const double *pos = (const double *) (r + parts->off_pos);
        h4[i] = make_double4(pos[0], pos[1], pos[2], want_mass ? (double) *(const float *) (r + parts->off_mass) : 0.0);
        hf[i] = (uint8_t) (((*(const uint8_t *) (r + parts->off_type) & 0xf) << 4) | (low ? *(const uint8_t *) (r + parts->off_flags) & 7u : 0u));
        finite = finite && isfinite(pos[0]) && isfinite(pos[1]) && isfinite(pos[2]);
    }
    SHQ_CHECK(finite, SHQ_ERR_INVALID, "%s: non-finite particle position", sc.who);
    if(n > 0) {
        SHQ_HIP(hipMemcpyAsync(pm4, h4.data(), sizeof(double4) * n, hipMemcpyHostToDevice, ctx->stream));
        SHQ_HIP(hipMemcpyAsync(fl, hf.data(), (size_t) n, hipMemcpyHostToDevice, ctx->stream));
    }
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* the host vectors go out of scope */
    *d_posm = pm4;
    *d_flags = fl;
    return SHQ_OK;
}
