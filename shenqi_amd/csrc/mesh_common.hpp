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

/* ---- the slab operators (glass, zeldovich, uvbg: one x-slab of the mesh per rank, driven by shenqi_amd/dist.py) */

/* doubles per z row of the bespoke passes on a slab, 0 for a mesh size without them */
inline int slab_pitch(int N) { return fft3d_route(N).bespoke ? shq_fft3d_pitch(N) : 0; }

/* The twiddles of mesh size N in an operator's own buffer of the context (buf, and n: the size it holds): a PM at one mesh size and
 * an operator's mesh at another do not evict each other. */
inline int slab_twiddles(shq_context *ctx, DevBuf<double> &buf, int &n, int N, const double **tw)
{
    if(n != N) {
        SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* a pass of another size may still read the table */
        n = 0;
        SHQ_TRY(buf.reserve(2 * (size_t) N));
        SHQ_TRY(shq_fft3d_fill_twiddles(N, buf.ptr));
        n = N;
    }
    *tw = buf.ptr;
    return SHQ_OK;
}

/* The Y/Z passes of `nplanes` x planes [nplanes][N][zp] doubles, in place: direction 0 takes the int64 planes of a field deposited
 * with exponent `exp` (worth 2^(exp - 61) per unit) to the (y, z) half spectrum, direction 1 goes back to real space with that
 * factor (SLAB_EXP_ONE: 1).  d_packed (NULL: in place) is the all-to-all buffer [nranks][nplanes][N / nranks][zp / 2] complex that
 * the Y pass stores into on the way out and loads from on the way back. */
constexpr int SLAB_EXP_ONE = 61;

/* tw, twn: the operator's twiddle buffer and its size in the context, as members: ctx is checked here, not by the caller */
inline int slab_fft_yz(shq_context *ctx, const char *who, DevBuf<double> shq_context::*tw, int shq_context::*twn, int N, void *d_planes,
                       int nplanes, int direction, int exp, const void *d_packed, int nranks)
{
    SHQ_CHECK(ctx && d_planes, SHQ_ERR_INVALID, "%s: null argument", who);
    const int zp = slab_pitch(N);
    SHQ_CHECK(zp > 0, SHQ_ERR_INVALID, "%s: mesh size %d has no bespoke FFT", who, N);
    SHQ_CHECK(nplanes > 0 && nplanes <= N && (direction == 0 || direction == 1) && exp > -900 && exp < 900, SHQ_ERR_INVALID, "%s: bad arguments", who);
    SHQ_CHECK(!d_packed || (nranks >= 1 && N % nranks == 0), SHQ_ERR_INVALID, "%s: %d ranks do not divide the mesh", who, nranks);
    SHQ_HIP(hipSetDevice(ctx->device));
    shq_fft_opts o;
    SHQ_TRY(slab_twiddles(ctx, ctx->*tw, ctx->*twn, N, &o.tw));
    o.nslab = nplanes;
    o.packed = (double *) const_cast<void *>(d_packed);
    o.nranks = d_packed ? nranks : 1;
    const shq_fft_stage st =
        direction == 0 ? (d_packed ? SHQ_FFT_YZ_FORWARD_PACKED : SHQ_FFT_YZ_FORWARD) : (d_packed ? SHQ_FFT_YZ_INVERSE_PACKED : SHQ_FFT_YZ_INVERSE);
    return shq_fft3d_run(ctx, (double *) d_planes, N, zp, st, direction == 0, ldexp(1.0, exp - 61), nullptr, 0, 0, o);
}

/* a particle window [nalloc][N][..]: the own planes [plane0, plane0 + nplanes) and one more behind them, or the whole periodic mesh */
inline bool slab_window_ok(int N, int plane0, int nplanes, int nalloc)
{
    return nplanes > 0 && nplanes <= N && plane0 >= 0 && plane0 < N && nalloc == (nplanes == N ? N : nplanes + 1);
}

/* The out-of-slab flag of a window kernel: `nflags` ints of an operator's own buffer zeroed on the stream before the launch, one of
 * them read after it - which synchronises. */
inline int slab_flag_reset(shq_context *ctx, DevBuf<int> &flag, size_t nflags = 1)
{
    SHQ_TRY(flag.reserve(nflags));
    SHQ_HIP(hipMemsetAsync(flag.ptr, 0, nflags * sizeof(int), ctx->stream));
    return SHQ_OK;
}

inline int slab_flag_read(shq_context *ctx, const int *d_flag, int *oob)
{
    *oob = 0;
    SHQ_HIP(hipMemcpyAsync(oob, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
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
