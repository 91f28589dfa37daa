/* fft3d.hip — bespoke in-place 3-D real FFT pipeline for the PM mesh on gfx950.
 *
 * Replaces the reference's heffte/cuFFT r2c + c2r (libgadget/petapm.cpp:49-71) and the separate
 * transfer-function sweep (pm_apply_transfer_function, petapm.cpp:1258-1298) for mesh sizes
 * N = 2^a 3^b 5^c up to 1536 (the compiled list is in shq_fft3d_supported).  rocFFT spends 6 memory passes per 3-D transform (3 FFT + 3
 * transpose kernels, 8.4 + 9.7 ms at 768^3); this pipeline needs FIVE passes for the whole
 * forward -> Green's function -> inverse sequence, each one read + one write of the mesh:
 *
 *   Z fwd : rows along z, two real rows per complex FFT (two-for-one), int64 fixed-point deposit
 *           converted on load (fuses pm_convert_kernel)            real [x][y][z] -> half spectrum
 *   Y fwd : lines along y, tiles of 4 adjacent z' columns (64-byte row segments)
 *   X     : lines along x: forward FFT, potential_transfer (gravpm.cpp:378-444) on the line while it
 *           sits in LDS, inverse FFT (fuses pm_green_kernel and saves a whole read+write pass)
 *   Y inv, Z inv (c2r, two-for-one).
 *
 * Every 1-D transform is a Stockham autosort FFT in LDS (radix 16 in registers while it divides,
 * then 4, 2 and a final 3): each stage reads its butterflies' inputs into registers, barrier, writes
 * the outputs to the same buffer, barrier — one LDS buffer per line (N+1 elements: the +1
 * de-conflicts the four column lines of a tile); the twiddle table sits in LDS next to the lines.
 * Workgroups are persistent and prefetch their next tile into registers (see below).
 * Unscaled in both directions, like FFTW/heffte.
 * The z pitch of the mesh is padded to a multiple of 4 complex values so that every 4-column row
 * segment is one aligned 64-byte chunk.
 */
#include "common.hpp"
#include <math.h>
#include <stdlib.h>

namespace {

#ifndef FFT_C
#define FFT_C 4        /* complex lines per workgroup */
#endif
/* threads per workgroup: 256, two workgroups per CU, up to Nmesh 768; above that one tile + tables no longer fit the LDS twice, and a
 * 256-thread workgroup would be one wave per SIMD holding 250-500 registers: 512 threads (the same two waves per SIMD, half the tile
 * elements per thread).  N is the mesh size wherever the macro is used. */
__host__ __device__ constexpr int fft_threads(int N) { return N > 768 ? 512 : 256; }
/* waves per SIMD the tile passes of the transposing pipeline are compiled for: the Y passes run three workgroups of four waves per CU up
 * to Nmesh 768 (a tile + its 48 twiddles take 53 KB of the CU's 160, and the passes fit 168 registers: 3-4 % faster than two in a
 * same-box A/B); the X pass keeps its Green's function factors in LDS and two workgroups (with the factors read from global memory and
 * three workgroups it ran 2.44 against 2.09 ms); above 768 the workgroups have eight waves and the bound stays at two per SIMD
 * (four - a 128-register budget - made the 1200 mesh spill: 208 ms for its five passes instead of 44).  The two halves of the X pass
 * (MODES 3 and 4, fft_t_tile) keep the fused pass's two: their P(k) histogram takes 3 N doubles of LDS beside the tile */
__host__ __device__ constexpr int fft_tile_waves(int N, int MODE) { return ((MODE == 0 || MODE == 1) && N <= 768) ? 3 : 2; }
#ifndef FFT_T
#define FFT_T fft_threads(N)
#endif
/* Element i of a line sits at LDS slot lx(i) = i + i / 16 (SHQ_FFT_PAD): the first radix-16 stage writes its outputs 16 elements
 * apart — 256 bytes, two full sweeps of the 32 store banks, so the eight lanes a ds_write_b128 serves per cycle all meet in the same
 * banks.  With one slot of padding per 16 elements consecutive lanes land 272 bytes apart, 16 bytes further along the banks each.
 * (SQ_LDS_BANK_CONFLICT was 60 % of SQ_LDS_IDX_ACTIVE.)  The stages split every index into a per-thread part and a compile-time
 * part without a carry between them, so that lx(t + c) = lx(t) + lx(c) and the sixteen accesses of a butterfly stay base register +
 * immediate offset (with lx(t + c) computed per access the passes need 244-269 VGPRs and lose a workgroup per CU).  The line stride
 * stays = 1 (mod 8) slots, which keeps the tile's transposed landing and leaving as they were. */
#ifndef SHQ_FFT_PAD
#define SHQ_FFT_PAD 1
#endif
/* the padding is used for the mesh sizes whose every stage splits that way (768 = 16 16 3, 1024 = 16 16 4, 1536 = 16 16 2 3, ...); the
 * others (384 = 16 4 2 3, 960 = 16 4 3 5, ...) keep the plain layout */
__host__ __device__ constexpr int fft_radix(int n) { return n % 16 == 0 ? 16 : (n % 4 == 0 ? 4 : (n % 2 == 0 ? 2 : (n % 3 == 0 ? 3 : 5))); }
__host__ __device__ constexpr bool fft_pad_ok(int N)
{
    if(!SHQ_FFT_PAD)
        return false;
    int n = N, s = 1;
    while(n > 1) {
        const int R = fft_radix(n), m = n / R;
        if((s * m) % 16 != 0 || !(s % 16 == 0 || ((s * R) % 16 == 0 && s * R <= 16)))
            return false;
        n = m;
        s *= R;
    }
    return true;
}
template <int N> __host__ __device__ constexpr int lx(int i) { return fft_pad_ok(N) ? i + (i >> 4) : i; }
/* Twiddles (round 4).  A butterfly of the stage (n, s, R) at position p multiplies its output k by w_N^(k p s).  Only w_N^(p s) is read
 * from the table, the powers follow by repeated multiplication (k <= 15: a dozen rounding errors of 1e-16 on factors of modulus one,
 * far inside the transforms' own error; every transform in the library takes its twiddles this way, so the pipelines that are
 * compared bit for bit still agree) - fifteen LDS reads and thirty registers less per radix-16 butterfly, and the table shrinks from
 * N entries to max over the stages of (m - 1) s + 1 (48 at 768): with 12 KB less LDS a tile pass fits THREE workgroups per CU. */
__host__ __device__ constexpr int fft_twn(int N)
{
    int n = N, s = 1, mx = 0;
    while(n > 1) {
        const int R = fft_radix(n), m = n / R;
        if((m - 1) * s > mx)
            mx = (m - 1) * s;
        n = m;
        s *= R;
    }
    return mx + 1;
}
__host__ __device__ constexpr int fft_ls(int N)
{
    const int last = fft_pad_ok(N) ? (N - 1) + ((N - 1) >> 4) : N - 1;
    return last + 1 + (9 - (last + 1) % 8) % 8;
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 conj2(double2 a) { return make_double2(a.x, -a.y); }
/* multiply by -i (forward) or +i (inverse) */
template <int DIR> __device__ __forceinline__ double2 rot(double2 a) { return DIR < 0 ? make_double2(a.y, -a.x) : make_double2(-a.y, a.x); }
template <int DIR> __device__ __forceinline__ double2 tw(const double2 *__restrict__ W, int idx)
{
    const double2 w = W[idx];
    return DIR < 0 ? w : conj2(w);
}
/* exp(DIR * 2 pi i m / 16) for the in-register radix-16 butterfly */
template <int DIR, int M> __device__ __forceinline__ double2 w16()
{
    constexpr double c[16] = {1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173, 0.0,
                              -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128673848, -1.0,
                              -0.92387953251128673848, -0.70710678118654752440, -0.38268343236508977173, 0.0,
                              0.38268343236508977173, 0.70710678118654752440, 0.92387953251128673848};
    constexpr double sn[16] = {0.0, 0.38268343236508977173, 0.70710678118654752440, 0.92387953251128673848, 1.0,
                               0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173, 0.0,
                               -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128673848, -1.0,
                               -0.92387953251128673848, -0.70710678118654752440, -0.38268343236508977173};
    return make_double2(c[M & 15], (DIR < 0 ? -1.0 : 1.0) * sn[M & 15]);
}

template <int DIR> __device__ __forceinline__ void bfly4(double2 &a0, double2 &a1, double2 &a2, double2 &a3)
{
    const double2 t0 = cadd(a0, a2), t1 = csub(a0, a2);
    const double2 t2 = cadd(a1, a3), t3 = rot<DIR>(csub(a1, a3));
    a0 = cadd(t0, t2);
    a1 = cadd(t1, t3);
    a2 = csub(t0, t2);
    a3 = csub(t1, t3);
}

/* b[k] = sum_j a[j] w16^(jk), in place, output in natural order k = k1 + 4 k0 stored at a[k] */
template <int DIR> __device__ __forceinline__ void bfly16(double2 (&a)[16])
{
    /* j = j0 + 4 j1: radix-4 over j1 for every j0 -> t[j0][k1] stored at a[j0 + 4 k1] */
#pragma unroll
    for(int j0 = 0; j0 < 4; j0++)
        bfly4<DIR>(a[j0], a[j0 + 4], a[j0 + 8], a[j0 + 12]);
    /* twiddle w16^(j0 k1) */
    a[1 + 4] = cmul(a[1 + 4], w16<DIR, 1>());
    a[2 + 4] = cmul(a[2 + 4], w16<DIR, 2>());
    a[3 + 4] = cmul(a[3 + 4], w16<DIR, 3>());
    a[1 + 8] = cmul(a[1 + 8], w16<DIR, 2>());
    a[2 + 8] = cmul(a[2 + 8], w16<DIR, 4>());
    a[3 + 8] = cmul(a[3 + 8], w16<DIR, 6>());
    a[1 + 12] = cmul(a[1 + 12], w16<DIR, 3>());
    a[2 + 12] = cmul(a[2 + 12], w16<DIR, 6>());
    a[3 + 12] = cmul(a[3 + 12], w16<DIR, 9>());
    /* radix-4 over j0 for every k1: b[k1 + 4 k0] */
#pragma unroll
    for(int k1 = 0; k1 < 4; k1++)
        bfly4<DIR>(a[4 * k1], a[4 * k1 + 1], a[4 * k1 + 2], a[4 * k1 + 3]);
    /* now a[4 k1 + k0] holds b[k1 + 4 k0]: transpose the 4x4 index to natural order */
#pragma unroll
    for(int k1 = 0; k1 < 4; k1++)
#pragma unroll
        for(int k0 = k1 + 1; k0 < 4; k0++) {
            const double2 tmp = a[4 * k1 + k0];
            a[4 * k1 + k0] = a[4 * k0 + k1];
            a[4 * k0 + k1] = tmp;
        }
}

/* One Stockham stage of radix R on FFT_C lines of length N held in LDS with line stride N + 1.
 * n = current sub-transform length, s = stride (product of the radices already applied); all are
 * compile-time constants, so the index arithmetic folds into shifts and constant multiplies. */
struct NoLoadOp {
    __device__ __forceinline__ double2 operator()(int, int, double2 v) const { return v; }
};

template <int N, int n, int s, int R, int DIR, typename StoreOp = NoLoadOp>
__device__ __forceinline__ void fft_stage(double2 *buf, const double2 *__restrict__ W, const StoreOp op = StoreOp())
{
    constexpr int LS = fft_ls(N);
    constexpr int m = n / R;
    constexpr int nb = N / R;               /* butterflies per line */
    constexpr int total = FFT_C * nb;
    constexpr int K = (total + FFT_T - 1) / FFT_T;
    double2 v[K][R];
#pragma unroll
    for(int kk = 0; kk < K; kk++) {
        const int i = threadIdx.x + kk * FFT_T;
        if(i < total) {
            const int line = i / nb, b = i - line * nb;
            const int p = b / s, q = b - p * s;
            /* s m j is a multiple of 16 in every stage of the 16 16 3 / 16 16 ... sequences: no carry into the padding term */
            const double2 *x = buf + line * LS + ((s * m) % 16 == 0 ? lx<N>(q + s * p) : 0);
#pragma unroll
            for(int j = 0; j < R; j++)
                v[kk][j] = x[(s * m) % 16 == 0 ? lx<N>(s * m * j) : lx<N>(q + s * p + s * m * j)];
            if(R == 2) {
                const double2 a0 = v[kk][0], a1 = v[kk][1];
                v[kk][0] = cadd(a0, a1);
                v[kk][1] = csub(a0, a1);
            } else if(R == 4) {
                bfly4<DIR>(v[kk][0], v[kk][1], v[kk][2], v[kk][3]);
            } else if(R == 3) {
                const double c = -0.5, sn = (DIR < 0 ? -1.0 : 1.0) * 0.86602540378443864676;
                const double2 a0 = v[kk][0];
                const double2 t1 = cadd(v[kk][1], v[kk][2]);
                const double2 t2 = make_double2(a0.x + c * t1.x, a0.y + c * t1.y);
                const double2 d = csub(v[kk][1], v[kk][2]);
                const double2 t3 = make_double2(-sn * d.y, sn * d.x); /* i * sn * d */
                v[kk][0] = cadd(a0, t1);
                v[kk][1] = cadd(t2, t3);
                v[kk][2] = csub(t2, t3);
            } else if(R == 5) {
                /* y_k = sum_j x_j w5^(jk), w5 = exp(DIR 2 pi i / 5) */
                const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410; /* cos 72, cos 144 */
                const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;  /* sin 72, sin 144 */
                const double2 x0 = v[kk][0];
                const double2 t1 = cadd(v[kk][1], v[kk][4]), t2 = cadd(v[kk][2], v[kk][3]);
                const double2 t3 = csub(v[kk][1], v[kk][4]), t4 = csub(v[kk][2], v[kk][3]);
                const double2 a1 = make_double2(x0.x + c1 * t1.x + c2 * t2.x, x0.y + c1 * t1.y + c2 * t2.y);
                const double2 a2 = make_double2(x0.x + c2 * t1.x + c1 * t2.x, x0.y + c2 * t1.y + c1 * t2.y);
                const double2 b1 = make_double2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y);
                const double2 b2 = make_double2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y);
                /* DIR < 0: y1 = a1 - i b1, y4 = a1 + i b1, y2 = a2 - i b2, y3 = a2 + i b2; conjugated for DIR > 0 */
                const double sg = DIR < 0 ? 1.0 : -1.0;
                v[kk][0] = make_double2(x0.x + t1.x + t2.x, x0.y + t1.y + t2.y);
                v[kk][1] = make_double2(a1.x + sg * b1.y, a1.y - sg * b1.x);
                v[kk][4] = make_double2(a1.x - sg * b1.y, a1.y + sg * b1.x);
                v[kk][2] = make_double2(a2.x + sg * b2.y, a2.y - sg * b2.x);
                v[kk][3] = make_double2(a2.x - sg * b2.y, a2.y + sg * b2.x);
            } else {
                bfly16<DIR>(reinterpret_cast<double2(&)[16]>(v[kk]));
            }
            if(m > 1) { /* w_n^(p k); the last stage (m == 1) has p == 0 */
                const double2 w1 = tw<DIR>(W, p * s);
                double2 wk = w1;
                v[kk][1] = cmul(v[kk][1], wk);
#pragma unroll
                for(int k = 2; k < R; k++) {
                    wk = cmul(wk, w1);
                    v[kk][k] = cmul(v[kk][k], wk);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for(int kk = 0; kk < K; kk++) {
        const int i = threadIdx.x + kk * FFT_T;
        if(i < total) {
            const int line = i / nb, b = i - line * nb;
            const int p = b / s, q = b - p * s;
            /* s k is a multiple of 16 (s % 16 == 0), or q + s k stays below 16 under a thread part that is a multiple of 16 */
            constexpr bool SPLIT = s % 16 == 0 || ((s * R) % 16 == 0 && s * R <= 16);
            double2 *y = buf + line * LS + (SPLIT ? lx<N>(s % 16 == 0 ? q + s * R * p : s * R * p) : 0);
#pragma unroll
            for(int k = 0; k < R; k++)
                y[SPLIT ? (s % 16 == 0 ? lx<N>(s * k) : q + s * k) : lx<N>(q + s * R * p + s * k)] = op(line, q + s * R * p + s * k, v[kk][k]);
        }
    }
    __syncthreads();
}

/* radix sequence: 16 while possible, then 4, 2, and a final 3 */
template <int N, int n, int s, int DIR> struct Stages {
    template <typename StoreOp> static __device__ __forceinline__ void run(double2 *buf, const double2 *__restrict__ W, const StoreOp op)
    {
        constexpr int R = n % 16 == 0 ? 16 : (n % 4 == 0 ? 4 : (n % 2 == 0 ? 2 : (n % 3 == 0 ? 3 : 5)));
        static_assert(n % R == 0, "mesh size must be 2^a 3^b 5^c");
        if constexpr(n / R > 1) {
            fft_stage<N, n, s, R, DIR>(buf, W);
            Stages<N, n / R, s * R, DIR>::run(buf, W, op);
        } else
            fft_stage<N, n, s, R, DIR, StoreOp>(buf, W, op); /* the hook filters the outputs of the last stage */
    }
};

/* op(line, index, value) filters every output element as the last stage stores it */
template <int N, int DIR, typename StoreOp = NoLoadOp>
__device__ __forceinline__ void fft_lines(double2 *buf, const double2 *__restrict__ W, const StoreOp op = StoreOp())
{
#ifdef SHQ_FFT_PROBE_NOCOMPUTE /* timing probe only (wrong results): what a pass costs without its transforms */
    __syncthreads();
#else
    Stages<N, N, 1, DIR>::run(buf, W, op);
#endif
}

/* ---- persistent workgroups -------------------------------------------------------------------------
 * Every pass runs as many workgroups as fit on the chip at once; workgroup b takes tiles b, b + G,
 * b + 2G ...  The twiddle table lives in LDS behind the line buffers (loaded once per workgroup), so
 * the FFT stages touch no global memory at all, and the NEXT tile is fetched into registers right
 * after the current one has landed in LDS: its HBM latency hides behind the LDS work.  (Measured
 * before: 70-80 % of wave cycles waiting, 15 dependent twiddle loads per radix-16 stage.)
 * The prefetch of the last iteration re-reads the workgroup's own tile instead of branching around
 * the loads, which keeps the loop-carried registers free of copies (and of an early s_waitcnt). */
template <int N> __device__ __forceinline__ double2 *lds_twiddles(double2 *buf, const double2 *__restrict__ W)
{
    double2 *Wl = buf + FFT_C * fft_ls(N);
    for(int i = threadIdx.x; i < fft_twn(N); i += FFT_T)
        Wl[i] = W[i];
    return Wl;
}

/* ---- pass Z forward: two real rows -> two half spectra, in place ---------------------------------
 * mesh: [nrows][zp] doubles (zp = pitch, >= N + 2).  Workgroup tile = FFT_C complex lines = 2 FFT_C rows. */
template <int N, bool FROM_I64>
__global__ __launch_bounds__(FFT_T) void fft_pass_z_fwd(double *mesh, const int ntot, const int zp,
                                                        const double2 *__restrict__ W, const double inv_scale)
{
    extern __shared__ double2 buf[];
    constexpr int LS = fft_ls(N), H = N / 2, Nc = N / 2 + 1;
    constexpr int E = (FFT_C * H + FFT_T - 1) / FFT_T; /* a thread takes the elements z, z + 1 of BOTH real rows of a line: see fft_t_z_fwd */
    constexpr bool EXACT = E * FFT_T == FFT_C * H;
    double2 *Wl = lds_twiddles<N>(buf, W);
    double2 *cm = reinterpret_cast<double2 *>(mesh);
    const int zpc = zp / 2;
    double pa[E], pb[E], pc[E], pd[E];
#define FFT_FETCH(T_)                                                                            \
    _Pragma("unroll") for(int i = 0; i < E; i++)                                                 \
    {                                                                                            \
        const int e_ = threadIdx.x + i * FFT_T, e = (EXACT || e_ < FFT_C * H) ? e_ : 0; /* no branch around the loads: see fft_t_z_inv */ \
        { \
            const int l_ = e / H;                                                                \
            const long long row = (long long) (T_) * (2 * FFT_C) + 2 * l_;                       \
            const double2 v_ = cm[row * zpc + (e - l_ * H)], w_ = cm[(row + 1) * zpc + (e - l_ * H)]; \
            pa[i] = v_.x;                                                                        \
            pb[i] = v_.y;                                                                        \
            pc[i] = w_.x;                                                                        \
            pd[i] = w_.y;                                                                        \
        }                                                                                        \
    }
    int t = blockIdx.x;
    if(t >= ntot)
        return;
    FFT_FETCH(t)
    while(true) {
#pragma unroll
        for(int i = 0; i < E; i++) {
            const int e = threadIdx.x + i * FFT_T;
            if(EXACT || e < FFT_C * H) {
                const int l = e / H, z = 2 * (e - l * H);
                double a = pa[i], b = pb[i], c = pc[i], d = pd[i];
                if(FROM_I64) {
                    a = (double) __double_as_longlong(a) * inv_scale;
                    b = (double) __double_as_longlong(b) * inv_scale;
                    c = (double) __double_as_longlong(c) * inv_scale;
                    d = (double) __double_as_longlong(d) * inv_scale;
                }
                buf[l * LS + lx<N>(z)] = make_double2(a, c);
                buf[l * LS + lx<N>(z + 1)] = make_double2(b, d);
            }
        }
        __syncthreads();
        const int tn = t + (int) gridDim.x;
        const bool more = tn < ntot;
        const int tf = more ? tn : t;
        FFT_FETCH(tf)
        fft_lines<N, -1>(buf, Wl);
        /* separate the two real transforms: XA[k] = (Z[k] + conj Z[N-k]) / 2, XB[k] = -i (Z[k] - conj Z[N-k]) / 2 */
        const long long row0 = (long long) t * (2 * FFT_C);
        for(int e = threadIdx.x; e < FFT_C * Nc; e += FFT_T) {
            const int l = e / Nc, k = e - l * Nc;
            const double2 zk = buf[l * LS + lx<N>(k)];
            const double2 zn = conj2(buf[l * LS + lx<N>(k == 0 ? 0 : N - k)]);
            const double2 xa = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y + zn.y));
            const double2 d = make_double2(0.5 * (zk.x - zn.x), 0.5 * (zk.y - zn.y));
            const double2 xb = make_double2(d.y, -d.x);
            const long long ra = row0 + 2 * l;
            cm[ra * zpc + k] = xa;
            cm[(ra + 1) * zpc + k] = xb;
        }
        if(!more)
            break;
        __syncthreads(); /* everyone has read its results out of LDS before the next tile lands there */
        t = tn;
    }
#undef FFT_FETCH
}

/* ---- pass Z inverse (c2r): two half spectra -> two real rows, in place -------------------------------- */
template <int N>
__global__ __launch_bounds__(FFT_T) void fft_pass_z_inv(double *mesh, const int ntot, const int zp, const double2 *__restrict__ W)
{
    extern __shared__ double2 buf[];
    constexpr int LS = fft_ls(N), H = N / 2, Nc = N / 2 + 1;
    constexpr int E = (FFT_C * Nc + FFT_T - 1) / FFT_T;
    double2 *Wl = lds_twiddles<N>(buf, W);
    double2 *cm = reinterpret_cast<double2 *>(mesh);
    const int zpc = zp / 2;
    double ax[E], ay[E], bx[E], by[E];
#define FFT_FETCH(T_)                                                                            \
    _Pragma("unroll") for(int i = 0; i < E; i++)                                                 \
    {                                                                                            \
        /* no branch around the loads (an unused slot reads the tile's first entry): see fft_t_z_inv */ \
        const int e_ = threadIdx.x + i * FFT_T, e = e_ < FFT_C * Nc ? e_ : 0;                    \
        const int l = e / Nc, k = e - l * Nc;                                                    \
        const long long ra = (long long) (T_) * (2 * FFT_C) + 2 * l;                             \
        const double2 xa_ = cm[ra * zpc + k], xb_ = cm[(ra + 1) * zpc + k];                      \
        ax[i] = xa_.x;                                                                           \
        ay[i] = xa_.y;                                                                           \
        bx[i] = xb_.x;                                                                           \
        by[i] = xb_.y;                                                                           \
    }
    int t = blockIdx.x;
    if(t >= ntot)
        return;
    FFT_FETCH(t)
    while(true) {
#pragma unroll
        for(int i = 0; i < E; i++) {
            const int e = threadIdx.x + i * FFT_T;
            asm volatile("" ::"v"(ax[i]), "v"(ay[i]), "v"(bx[i]), "v"(by[i])); /* every loaded half stays alive up to here: see fft_t_z_inv */
            if(e < FFT_C * Nc) {
                const int l = e / Nc, k = e - l * Nc;
                double2 xa = make_double2(ax[i], ay[i]), xb = make_double2(bx[i], by[i]);
                if(k == 0 || 2 * k == N) { /* a c2r transform ignores the imaginary part of the self-conjugate modes */
                    xa.y = 0;
                    xb.y = 0;
                }
                /* Z[k] = XA[k] + i XB[k];  Z[N-k] = conj(XA[k]) + i conj(XB[k]) */
                buf[l * LS + lx<N>(k)] = make_double2(xa.x - xb.y, xa.y + xb.x);
                if(k > 0 && 2 * k < N)
                    buf[l * LS + lx<N>(N - k)] = make_double2(xa.x + xb.y, -xa.y + xb.x);
            }
        }
        __syncthreads();
        const int tn = t + (int) gridDim.x;
        const bool more = tn < ntot;
        const int tf = more ? tn : t;
        FFT_FETCH(tf)
        fft_lines<N, +1>(buf, Wl);
        const long long row0 = (long long) t * (2 * FFT_C);
        /* a thread takes the elements z, z + 1 of one line (two 16-byte LDS reads, consecutive lanes 32 bytes apart: no bank conflicts;
         * the 8-byte reads of one row's real parts, 32 bytes apart, met four to a bank) and stores them to the line's two real rows */
        for(int e = threadIdx.x; e < FFT_C * H; e += FFT_T) {
            const int l = e / H, zz = e - l * H;
            const double2 u0 = buf[l * LS + lx<N>(2 * zz)], u1 = buf[l * LS + lx<N>(2 * zz + 1)];
            cm[(row0 + 2 * l) * zpc + zz] = make_double2(u0.x, u1.x);
            cm[(row0 + 2 * l + 1) * zpc + zz] = make_double2(u0.y, u1.y);
        }
        if(!more)
            break;
        __syncthreads();
        t = tn;
    }
#undef FFT_FETCH
}

/* ---- passes Y and X: complex lines with element stride `es` (in complex units), FFT_C adjacent columns.
 * MODE 0: forward only; 1: inverse only; 2: forward, Green's function, inverse (X pass of the PM).
 * MODES 3, 4 (fft_pass_strided only, the X pass of a y-slab): MODE 2 split in two as fft_t_tile's MODES 3, 4 split it (below). */
struct GreenArgs {
    const double *sinctab = nullptr; /* 1 / sinc^2(pi k / N) per mesh index */
    const double *gaxg = nullptr;    /* transposing pipeline: exp(-k_i^2 asmth2) sinctab[i]^2 per mesh index, in global memory (fft_gax_kernel) */
    double asmth2 = 0, pot_factor = 0;
    int y0 = 0;                      /* mesh index of outer = 0 in the X pass (y-slab of a distributed mesh) */
    /* PK != 0 (Y pass of a distributed mesh): the transposed side of the pass lives in `alt`, laid out as the all-to-all wants it,
     * [dest rank q][x plane][y inside q's slab][z']: line element y sits at alt + (y / nyl) qstride + outer alt_outer + (y % nyl) es */
    double2 *alt = nullptr;
    int nyl = 1;
    long long qstride = 0, alt_outer = 0;
    /* the split X pass of the transposing pipeline (fft_t_tile MODES 3 and 4): the caller's factor by integer k2 (entry k2 & fac_mask:
     * fac_mask = 0 with a one-entry table {1.0} when there is none), and the P(k) sums of powerspectrum_add_mode (ps = null: none) -
     * ps[0, N) power, [N, 2N) kk, [2N, 3N) modes (u64), ps[3N] norm; the bin of k2 is bintab[k2] (pm.hip, pm_power_prepare) */
    const double *modefac = nullptr;
    int fac_mask = 0;
    const int32_t *bintab = nullptr;
    double *ps = nullptr;
    int ncell = 1; /* MODE 5: the int N^3 every mode is divided by (uvbg.cpp:211-215 divide_by_ncell) */
    double2 *out = nullptr; /* fft_pass_strided MODES 5, 6, 8: the y-slab the result is stored into, laid out as the one it reads */
    int zel_axis = -1;      /* fft_pass_strided MODE 6: zel_transfer_mode's axis and c0; MODE 8: the axis of the glass's force */
    double zel_c0 = 0;
};

/* powerspectrum_add_mode (gravpm.cpp:323-356) of one mode into a workgroup's LDS histogram [3][N]: the operations of pm_power_kernel
 * (pm.hip).  The zero mode sets Norm; pad columns z > N / 2 are not modes. */
template <int N>
__device__ __forceinline__ void pk_add(double *hist, const GreenArgs &ga, double2 v, int x, int y, int z, int k2)
{
    if(z > N / 2)
        return;
    const double m = v.x * v.x + v.y * v.y;
    if(k2 == 0) {
        ga.ps[3 * N] = m;
        return;
    }
    const int kint = ga.bintab[k2];
    if(kint >= N)
        return;
    const double f = ga.sinctab[x] * ga.sinctab[y] * ga.sinctab[z];
    const double w = (z == 0 || z == N / 2) ? 1.0 : 2.0;
    atomicAdd(&hist[kint], w * m * f * f);
    atomicAdd(&hist[N + kint], w * sqrt((double) k2));
    atomicAdd(&hist[2 * N + kint], w);
}

/* Both power additions of a glass force (glass.hip, glass_power_kernel: the same operations per mode) into a workgroup's LDS histogram
 * [3][N]: measure_power_spectrum's with the deconvolution weight and potential_transfer's with weight 1 (glass.cpp:304), same bins. */
template <int N>
__device__ __forceinline__ void glass_pk_add(double *hist, const GreenArgs &ga, double2 v, int x, int y, int z, int k2)
{
    if(z > N / 2)
        return;
    const double m = v.x * v.x + v.y * v.y;
    if(k2 == 0) {
        ga.ps[3 * N] = m; /* Norm: both callers write the same value */
        return;
    }
    const int kint = ga.bintab[k2];
    if(kint >= N)
        return;
    const double f = ga.sinctab[x] * ga.sinctab[y] * ga.sinctab[z];
    const double w = (z == 0 || z == N / 2) ? 1.0 : 2.0;
    atomicAdd(&hist[kint], w * m * f * f + w * m);
    atomicAdd(&hist[N + kint], 2 * (w * sqrt((double) k2)));
    atomicAdd(&hist[2 * N + kint], 2 * w);
}

/* PK 0: in place.  PK 1: results stored into ga.alt in the packed (send) layout.  PK 2: input loaded from ga.alt in that layout.
 * The X pass of a y-slab split for a caller that needs the density spectrum between its halves (shq_pm_slab2_xforward / _xfinish):
 *   MODE 3: X forward, the spectrum written back in place; with ga.ps the P(k) sums of the density as the tile is stored.  y = ga.y0 +
 *           outer: only the rank whose slab holds y = 0 meets the zero mode and writes Norm (the others leave it 0).
 *   MODE 4: every mode times T[k2], then MODE 2's Green's factor with MODE 2's arithmetic - (v T) green, potential_transfer's order
 *           (gravpm.cpp:412-443) - as the tile lands in LDS; with ga.ps the P(k) sums of v T; then X inverse.  T = 1 gives MODE 2's
 *           bits: v * 1.0 is exact.  T[k2] of the next tile is gathered after the current tile's stages, as fft_t_tile does.
 *   MODE 5: the excursion-set filter on a y-slab (uvbg.hip, the sibling of fft_t_tile's MODE 5): reads a tile of the kept spectrum,
 *           every mode becomes (v / ncell) T[k2] - divide_by_ncell, then filter_pm (uvbg.cpp:211-250) - with no Green's function,
 *           then X inverse, stored OUT OF PLACE into the same place of ga.out: the kept spectrum is only read.
 *   MODE 6: the Zel'dovich transfer of one field on a y-slab (zeldovich.hip), MODE 5 with another factor: reads a tile of the kept
 *           Gaussian field, every mode becomes zel_transfer_mode(v, k2, k_axis, axis, T[k2], c0) - the one-rank kernel's function -
 *           then X inverse, stored out of place into ga.out.  A pad column (z > N / 2) passes as it is.
 *   MODE 7: the X forward of a glass force's density on a y-slab (glass.hip), MODE 3 with the glass's sums: with ga.ps both power
 *           additions of the reference per mode (glass_pk_add) as the tile is stored.  The spectrum's bits do not depend on ga.ps.
 *   MODE 8: the glass's potential and force transfer of one axis on a y-slab, the sibling of MODE 6: reads a tile of the kept density
 *           spectrum, every mode becomes v * (pot_factor * (1.0 / k2) * f * f) with f = 1, the zero mode 0, then (-v.y fa, v.x fa)
 *           with fa = ga.modefac[index along ga.zel_axis] (N entries, held in LDS where MODE 2 keeps its factors) - the operations of
 *           glass_transfer_kernel - then X inverse, stored out of place into ga.out.  A pad column (z > N / 2) is stored as 0.
 * MODES 3, 4, 7 with ga.ps keep a P(k) histogram [3][N] in LDS behind the tables (3 N doubles more), flushed once per workgroup. */
template <int N, int MODE, int PK = 0>
__global__ __launch_bounds__(FFT_T) void fft_pass_strided(double2 *cm, const long long es, const long long outer_stride,
                                                          const int ntiles, const int ntot, const double2 *__restrict__ W,
                                                          const GreenArgs ga, const unsigned xcdk, const int tile0 = 0)
{
    extern __shared__ double2 buf[];
    constexpr int LS = fft_ls(N);
    constexpr int E = (FFT_C * N + FFT_T - 1) / FFT_T; /* tile elements per thread */
    constexpr bool EXACT = E * FFT_T == FFT_C * N;
    double2 *Wl = lds_twiddles<N>(buf, W);
    double *gax = reinterpret_cast<double *>(Wl + fft_twn(N)); /* MODES 2, 4: per-axis factor of the Green's function */
    if(MODE == 2 || MODE == 4)
        for(int i = threadIdx.x; i < N; i += FFT_T) {
            const int k = i <= N / 2 ? i : i - N;
            const double sc = ga.sinctab[i];
            gax[i] = exp(-(double) k * (double) k * ga.asmth2) * sc * sc;
        }
    /* MODES 3, 4 with ga.ps: the histogram behind the tables; the barrier after the first tile lands orders the zeroing */
    double *hist = MODE == 4 ? gax + N : gax;
    const bool pk = (MODE == 3 || MODE == 4 || MODE == 7) && ga.ps;
    if(pk)
        for(int i = threadIdx.x; i < 3 * N; i += FFT_T)
            hist[i] = 0;
    if(MODE == 8) { /* the tile lands through this table, before the first barrier of the loop */
        for(int i = threadIdx.x; i < N; i += FFT_T)
            gax[i] = ga.modefac[i];
        __syncthreads();
    }
    /* XCD-chunked workgroup order: neighbouring column tiles share 128-byte lines (a tile row is 64
     * bytes), so they should run on the same XCD at about the same time and find the other half in its L2. */
    const unsigned vb = xcd_block(blockIdx.x, gridDim.x, xcdk);
    double prx[E], pry[E];
    double tfac[MODE == 4 || MODE == 5 || MODE == 6 ? E : 1]; /* MODES 4, 5, 6: T[k2] of the prefetched tile's modes */
#define FFT_FETCH(BASE, ABASE)                                                                   \
    _Pragma("unroll") for(int i = 0; i < E; i++)                                                 \
    {                                                                                            \
        const int e_ = threadIdx.x + i * FFT_T, e = (EXACT || e_ < FFT_C * N) ? e_ : 0; /* no branch around the loads: see fft_t_z_inv */ \
        { \
            const int r_ = e / FFT_C, c_ = e % FFT_C;                                            \
            const double2 t_ = PK == 2 ? (ABASE)[(long long) (r_ / ga.nyl) * ga.qstride + (long long) (r_ % ga.nyl) * es + c_] \
                                       : (BASE)[(long long) r_ * es + c_];                       \
            prx[i] = t_.x;                                                                       \
            pry[i] = t_.y;                                                                       \
        }                                                                                        \
    }
    /* MODES 4, 5, 6: T[k2] of the modes of tile (O_, TL_); a pad column (z > N / 2) reads entry 0, so k2 stays inside the table */
#define FFT_TFETCH(O_, TL_)                                                                      \
    if(MODE == 4 || MODE == 5 || MODE == 6) {                                                  \
        const int y_ = ga.y0 + (O_), ky_ = y_ <= N / 2 ? y_ : y_ - N;                            \
        _Pragma("unroll") for(int i = 0; i < E; i++)                                             \
        {                                                                                        \
            const int e_ = threadIdx.x + i * FFT_T, e = (EXACT || e_ < FFT_C * N) ? e_ : 0;     \
            const int x_ = e / FFT_C, z_ = (TL_) * FFT_C + e % FFT_C, kx_ = x_ <= N / 2 ? x_ : x_ - N; \
            const int k2_ = z_ <= N / 2 ? kx_ * kx_ + ky_ * ky_ + z_ * z_ : 0;                   \
            tfac[i] = ga.modefac[k2_ & ga.fac_mask];                                             \
        }                                                                                        \
    }
    int t = (int) vb;
    if(t >= ntot)
        return;
    /* a launch covers the column tiles [tile0, tile0 + ntiles) of every outer index (all of them, or one z' chunk of the chained
     * Y -> X -> Y sequence below) */
    int outer = t / ntiles, tile = tile0 + (t - outer * ntiles);
    double2 *base = cm + (long long) outer * outer_stride + (long long) tile * FFT_C;
    double2 *abase = PK ? ga.alt + (long long) outer * ga.alt_outer + (long long) tile * FFT_C : nullptr;
    FFT_FETCH(base, abase)
    FFT_TFETCH(outer, tile)
    while(true) {
        if(MODE == 4) {
            /* (v T) green: the tile lands multiplied by T (T[0] is not used: the zero mode is removed), then a rolled sweep over LDS
             * takes its P(k) and applies MODE 2's Green's factor */
            const int y = ga.y0 + outer, z0 = tile * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N) {
                    const int x = e / FFT_C, z = z0 + e % FFT_C;
                    const int kx = x <= N / 2 ? x : x - N;
                    const double tv = (z <= N / 2 && kx * kx + ky * ky + z * z != 0) ? tfac[i] : 1.0;
                    buf[(e % FFT_C) * LS + lx<N>(x)] = make_double2(prx[i] * tv, pry[i] * tv);
                }
            }
            __syncthreads();
            const double gy = gax[y] * ga.pot_factor, ky2 = (double) ky * (double) ky;
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T) {
                const int x = e / FFT_C, col = e % FFT_C, z = z0 + col;
                const int kx = x <= N / 2 ? x : x - N;
                double2 *p = buf + col * LS + lx<N>(x);
                const double2 v = *p;
                if(pk)
                    pk_add<N>(hist, ga, v, x, y, z, kx * kx + ky * ky + z * z);
                const double k2 = (double) kx * (double) kx + (ky2 + (double) z * (double) z); /* exact: < 2^53 */
                const double fac = (k2 == 0.0 || z > N / 2) ? 0.0 : gax[x] * gy * gax[z] / k2;
                *p = make_double2(v.x * fac, v.y * fac);
            }
        } else if(MODE == 5) {
            /* value /= total_n_cells, then value *= filter: a division and a multiplication, never contracted */
#pragma clang fp contract(off)
            const double nc = (double) ga.ncell;
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N)
                    buf[(e % FFT_C) * LS + lx<N>(e / FFT_C)] = make_double2((prx[i] / nc) * tfac[i], (pry[i] / nc) * tfac[i]);
            }
        } else if(MODE == 6) {
            const int y = ga.y0 + outer, z0 = tile * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N) {
                    const int x = e / FFT_C, z = z0 + e % FFT_C;
                    const int kx = x <= N / 2 ? x : x - N;
                    const int k2 = z <= N / 2 ? kx * kx + ky * ky + z * z : 0;
                    const int ka = ga.zel_axis == 0 ? kx : (ga.zel_axis == 1 ? ky : z);
                    buf[(e % FFT_C) * LS + lx<N>(x)] = zel_transfer_mode(make_double2(prx[i], pry[i]), k2, ka, ga.zel_axis, tfac[i], ga.zel_c0);
                }
            }
        } else if(MODE == 8) {
            /* potential_transfer and force_transfer (glass.cpp:285-342): products and a division, never contracted */
#pragma clang fp contract(off)
            const int y = ga.y0 + outer, z0 = tile * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N) {
                    const int x = e / FFT_C, z = z0 + e % FFT_C;
                    const int kx = x <= N / 2 ? x : x - N;
                    const long long k2 = (long long) kx * kx + (long long) ky * ky + (long long) z * z;
                    double2 v = make_double2(prx[i], pry[i]);
                    if(k2 == 0 || z > N / 2)
                        v = make_double2(0.0, 0.0);
                    else {
                        const double f = 1.0;
                        const double smth = 1.0 / k2;
                        const double pf = ga.pot_factor * smth * f * f;
                        v.x *= pf;
                        v.y *= pf;
                    }
                    const double fa = gax[ga.zel_axis == 0 ? x : (ga.zel_axis == 1 ? y : (z <= N / 2 ? z : 0))];
                    const double tmp0 = -v.y * fa;
                    const double tmp1 = v.x * fa;
                    buf[(e % FFT_C) * LS + lx<N>(x)] = make_double2(tmp0, tmp1);
                }
            }
        } else {
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N)
                    buf[(e % FFT_C) * LS + lx<N>(e / FFT_C)] = make_double2(prx[i], pry[i]);
            }
        }
        __syncthreads();
        const int tn = t + (int) gridDim.x;
        const bool more = tn < ntot;
        const int outer_n = more ? tn / ntiles : outer, tile_n = more ? tile0 + (tn - outer_n * ntiles) : tile;
        double2 *base_n = cm + (long long) outer_n * outer_stride + (long long) tile_n * FFT_C;
        double2 *abase_n = PK ? ga.alt + (long long) outer_n * ga.alt_outer + (long long) tile_n * FFT_C : nullptr;
        FFT_FETCH(base_n, abase_n)
        if(MODE == 0 || MODE == 3 || MODE == 7)
            fft_lines<N, -1>(buf, Wl);
        if(MODE == 2) {
            /* potential_transfer, gravpm.cpp:378-444, applied as the forward transform stores its last
             * stage (line index = kx, outer = y, column = z'); gax[i] = exp(-k_i^2 asmth2) sinctab[i]^2, so
             * the factor exp(-k^2 asmth2) f^2 / k^2 is a product of three table entries over k^2 */
            const int y = ga.y0 + outer, z0 = tile * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
            const double gy = gax[y] * ga.pot_factor, ky2 = (double) ky * (double) ky;
            auto green = [=](int col, int x, double2 v) {
                const int z = z0 + col;
                const int kx = x <= N / 2 ? x : x - N;
                const double k2 = (double) kx * (double) kx + (ky2 + (double) z * (double) z); /* exact: < 2^53 */
                const double fac = (k2 == 0.0 || z > N / 2) ? 0.0 : gax[x] * gy * gax[z] / k2;
                return make_double2(v.x * fac, v.y * fac);
            };
            fft_lines<N, -1>(buf, Wl, green);
            fft_lines<N, +1>(buf, Wl);
        }
        if(MODE == 1 || MODE == 4 || MODE == 5 || MODE == 6 || MODE == 8)
            fft_lines<N, +1>(buf, Wl);
        FFT_TFETCH(outer_n, tile_n)
        if(MODE == 3 || MODE == 7) { /* the spectrum back in place; the density's P(k) on the way (MODE 7: the glass's two additions) */
            const int y = ga.y0 + outer, z0 = tile * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T) {
                const int row = e / FFT_C, col = e - row * FFT_C;
                const double2 v = buf[col * LS + lx<N>(row)];
                base[(long long) row * es + col] = v;
                if(pk) {
                    const int kx = row <= N / 2 ? row : row - N;
                    if(MODE == 7)
                        glass_pk_add<N>(hist, ga, v, row, y, z0 + col, kx * kx + ky * ky + (z0 + col) * (z0 + col));
                    else
                        pk_add<N>(hist, ga, v, row, y, z0 + col, kx * kx + ky * ky + (z0 + col) * (z0 + col));
                }
            }
        } else {
            double2 *ob = MODE == 5 || MODE == 6 || MODE == 8 ? ga.out + (base - cm) : base; /* MODES 5, 6, 8: the same tile of the other y-slab */
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T) {
                const int row = e / FFT_C, col = e - row * FFT_C;
                if(PK == 1)
                    abase[(long long) (row / ga.nyl) * ga.qstride + (long long) (row % ga.nyl) * es + col] = buf[col * LS + lx<N>(row)];
                else
                    ob[(long long) row * es + col] = buf[col * LS + lx<N>(row)];
            }
        }
        if(!more)
            break;
        __syncthreads(); /* everyone has read its results out of LDS before the next tile lands there */
        t = tn;
        outer = outer_n;
        tile = tile_n;
        base = base_n;
        abase = abase_n;
    }
#undef FFT_FETCH
#undef FFT_TFETCH
    if(pk) { /* one atomic per non-empty bin, as pm_power_kernel */
        __syncthreads();
        unsigned long long *nmodes = reinterpret_cast<unsigned long long *>(ga.ps + 2 * N);
        for(int i = threadIdx.x; i < N; i += FFT_T)
            if(hist[2 * N + i] != 0) {
                atomicAdd(&ga.ps[i], hist[i]);
                atomicAdd(&ga.ps[N + i], hist[N + i]);
                atomicAdd(&nmodes[i], (unsigned long long) hist[2 * N + i]);
            }
    }
}

/* ---- the transposing pipeline (round 4; the undivided PM of shq_pm_run / shq_treepm_step) ------------------------------------
 * tools/copy_probe.hip moves the 768^3 mesh in the access shapes of the passes with nothing but 16-byte loads and stores:
 * contiguous 48 KB tiles both sides 1.25 ms (5.8 TB/s); one side in pieces of 512 / 256 / 128 / 64 B 1.27 / 1.38 / 1.50 / 1.57 ms;
 * BOTH sides in 64-byte pieces 6208 B apart (the Y passes above) 1.83-1.91 ms, 37 MB apart (the X pass) 2.2-2.4 ms - the passes above run
 * at those rates already (1.65 / 2.38 ms): what bounds them is the DRAM's row activations, one per 64-byte piece, not the FFT.
 * So the mesh changes its layout from pass to pass, between the mesh A and a scratch mesh B of the same size, such that one side of
 * every pass is a contiguous tile and only two of the ten sides are left with 64-byte pieces:
 *
 *   LY = [x][zb][y][4]   tile (x, zb) = the four z' columns 4 zb .. 4 zb + 3 of plane x, all y: N x 64 B contiguous
 *   LX = [y][zb][x][4]   tile (y, zb) likewise with the lines along x
 *
 *   Z fwd   A (real rows [x][y][z], int64 deposit)  -> B in LY: 8 rows in, per z' block one 512-byte piece (8 y x 4 z') out
 *   Y fwd   B tile (x, zb) contiguous               -> A in LX: row ky of the tile is a 64-byte piece
 *   X       A tile (ky, zb) contiguous: forward, potential_transfer, inverse  -> B in LY: row x is a 64-byte piece
 *   Y inv   B tile (x, zb) contiguous               -> the same tile of B, in place
 *   Z inv   B in LY, gathered in 512-byte pieces    -> A (real rows): the potential, where the deposit was
 *
 * The arithmetic - stages, twiddles, the two-for-one separation, the Green's function - is the functions above applied to the same
 * values in the same order: the potential mesh is bit-identical to the in-place pipeline's (a test compares the two). */
template <int N, bool FROM_I64>
__global__ __launch_bounds__(FFT_T) void fft_t_z_fwd(const double *mesh, double2 *__restrict__ out, const int ntot, const int zp,
                                                     const double2 *__restrict__ W, const double inv_scale)
{
    extern __shared__ double2 buf[];
    constexpr int LS = fft_ls(N), H = N / 2, Nc = N / 2 + 1;
    constexpr int E = (FFT_C * H + FFT_T - 1) / FFT_T; /* a thread takes the elements z, z + 1 of BOTH real rows of a line (the line's */
    constexpr bool EXACT = E * FFT_T == FFT_C * H;     /* entries z, z + 1 are then two 16-byte LDS stores; 8-byte stores 32 bytes apart */
    static_assert(FFT_C == 4, "the layouts are written for tiles of 4 lines"); /* met four to a bank) */
    double2 *Wl = lds_twiddles<N>(buf, W);
    const double2 *cm = reinterpret_cast<const double2 *>(mesh);
    const int zpc = zp / 2, nzb = zpc / 4;
    double pa[E], pb[E], pc[E], pd[E];
#define FFT_FETCH(T_)                                                                            \
    _Pragma("unroll") for(int i = 0; i < E; i++)                                                 \
    {                                                                                            \
        const int e_ = threadIdx.x + i * FFT_T, e = (EXACT || e_ < FFT_C * H) ? e_ : 0; /* no branch around the loads: see fft_t_z_inv */ \
        { \
            const int l_ = e / H;                                                                \
            const long long row = (long long) (T_) * (2 * FFT_C) + 2 * l_;                       \
            const double2 v_ = cm[row * zpc + (e - l_ * H)], w_ = cm[(row + 1) * zpc + (e - l_ * H)]; \
            pa[i] = v_.x;                                                                        \
            pb[i] = v_.y;                                                                        \
            pc[i] = w_.x;                                                                        \
            pd[i] = w_.y;                                                                        \
        }                                                                                        \
    }
    int t = blockIdx.x;
    if(t >= ntot)
        return;
    FFT_FETCH(t)
    while(true) {
#pragma unroll
        for(int i = 0; i < E; i++) {
            const int e = threadIdx.x + i * FFT_T;
            if(EXACT || e < FFT_C * H) {
                const int l = e / H, z = 2 * (e - l * H);
                double a = pa[i], b = pb[i], c = pc[i], d = pd[i];
                if(FROM_I64) {
                    a = (double) __double_as_longlong(a) * inv_scale;
                    b = (double) __double_as_longlong(b) * inv_scale;
                    c = (double) __double_as_longlong(c) * inv_scale;
                    d = (double) __double_as_longlong(d) * inv_scale;
                }
                buf[l * LS + lx<N>(z)] = make_double2(a, c);
                buf[l * LS + lx<N>(z + 1)] = make_double2(b, d);
            }
        }
        __syncthreads();
        const int tn = t + (int) gridDim.x;
        const bool more = tn < ntot;
        const int tf = more ? tn : t;
        FFT_FETCH(tf)
        fft_lines<N, -1>(buf, Wl);
        /* rows 8 t .. 8 t + 7 = plane x, rows y0 .. y0 + 7 (8 divides N).  Thread -> (zb, line pair l, column c): sixteen threads fill
         * one 512-byte piece [zb][y0 .. y0 + 7][4] with two stores each (rows y0 + 2 l and y0 + 2 l + 1) */
        const long long row0 = (long long) t * (2 * FFT_C);
        const int x = (int) (row0 / N), y0 = (int) (row0 - (long long) x * N);
        for(int e = threadIdx.x; e < 16 * nzb; e += FFT_T) {
            const int zb = e >> 4, l = (e >> 2) & 3, c = e & 3, k = 4 * zb + c;
            double2 xa = make_double2(0, 0), xb = make_double2(0, 0); /* the pad columns k >= Nc hold zeros */
            if(k < Nc) {
                const double2 zk = buf[l * LS + lx<N>(k)];
                const double2 zn = conj2(buf[l * LS + lx<N>(k == 0 ? 0 : N - k)]);
                xa = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y + zn.y));
                const double2 d = make_double2(0.5 * (zk.x - zn.x), 0.5 * (zk.y - zn.y));
                xb = make_double2(d.y, -d.x);
            }
            double2 *o = out + (((long long) x * nzb + zb) * N + (y0 + 2 * l)) * 4 + c;
            o[0] = xa;
            o[4] = xb;
        }
        if(!more)
            break;
        __syncthreads();
        t = tn;
    }
#undef FFT_FETCH
}

template <int N>
__global__ __launch_bounds__(FFT_T) void fft_t_z_inv(const double2 *__restrict__ in, double *mesh, const int ntot, const int zp, const double2 *__restrict__ W)
{
    extern __shared__ double2 buf[];
    constexpr int LS = fft_ls(N), H = N / 2, Nc = N / 2 + 1;
    double2 *Wl = lds_twiddles<N>(buf, W);
    double2 *cm = reinterpret_cast<double2 *>(mesh);
    const int zpc = zp / 2, nzb = zpc / 4;
    constexpr int EMAX = (16 * ((N / 2 + 1 + 3) / 4) + FFT_T - 1) / FFT_T; /* 16 (zb, l, c) slots per z' block of the unpadded spectrum... */
    const int nslots = 16 * nzb;                                           /* ...the pitch may hold more blocks: those are skipped */
    double ax[EMAX], ay[EMAX], bx[EMAX], by[EMAX];
#define FFT_FETCH(T_)                                                                            \
    {                                                                                            \
        const long long row0_ = (long long) (T_) * (2 * FFT_C);                                  \
        const int x_ = (int) (row0_ / N), y0_ = (int) (row0_ - (long long) x_ * N);              \
        _Pragma("unroll") for(int i = 0; i < EMAX; i++)                                          \
        {                                                                                        \
            const int e = threadIdx.x + i * FFT_T;                                               \
            const int zb = e >> 4, l = (e >> 2) & 3, c = e & 3, k = 4 * zb + c;                  \
            /* no branch around the loads: an unused slot reads the tile's first entry instead.  With the loads under the slot's  \
             * condition the compiler ended every pair with s_waitcnt vmcnt(0) (the values pass into loop-carried registers at the \
             * join) and the "prefetch" was seven round trips to memory one after the other */                                     \
            const bool ok_ = e < nslots && k < Nc;                                               \
            const double2 *p_ = in + (((long long) x_ * nzb + (ok_ ? zb : 0)) * N + (y0_ + 2 * l)) * 4 + (ok_ ? c : 0); \
            const double2 xa_ = p_[0], xb_ = p_[4];                                              \
            ax[i] = xa_.x;                                                                       \
            ay[i] = xa_.y;                                                                       \
            bx[i] = xb_.x;                                                                       \
            by[i] = xb_.y;                                                                       \
        }                                                                                        \
    }
    int t = blockIdx.x;
    if(t >= ntot)
        return;
    FFT_FETCH(t)
    while(true) {
#pragma unroll
        for(int i = 0; i < EMAX; i++) {
            const int e = threadIdx.x + i * FFT_T;
            const int zb = e >> 4, l = (e >> 2) & 3, c = e & 3, k = 4 * zb + c;
            /* all four components stay alive up to here: the last slot group's imaginary parts are never used (its only column is
             * N / 2), and the compiler handed their halves of the in-flight 16-byte loads to the first stage's temporaries - a write
             * after write that made the stage wait for the whole prefetch */
            asm volatile("" ::"v"(ax[i]), "v"(ay[i]), "v"(bx[i]), "v"(by[i]));
            if(e < nslots && k < Nc) {
                double2 xa = make_double2(ax[i], ay[i]), xb = make_double2(bx[i], by[i]);
                if(k == 0 || 2 * k == N) {
                    xa.y = 0;
                    xb.y = 0;
                }
                buf[l * LS + lx<N>(k)] = make_double2(xa.x - xb.y, xa.y + xb.x);
                if(k > 0 && 2 * k < N)
                    buf[l * LS + lx<N>(N - k)] = make_double2(xa.x + xb.y, -xa.y + xb.x);
            }
        }
        __syncthreads();
        const int tn = t + (int) gridDim.x;
        const bool more = tn < ntot;
        const int tf = more ? tn : t;
        FFT_FETCH(tf)
        fft_lines<N, +1>(buf, Wl);
        const long long row0 = (long long) t * (2 * FFT_C);
        /* a thread takes the elements z, z + 1 of one line (two 16-byte LDS reads, consecutive lanes 32 bytes apart: no bank conflicts;
         * the 8-byte reads of one row's real parts, 32 bytes apart, met four to a bank) and stores them to the line's two real rows */
        for(int e = threadIdx.x; e < FFT_C * H; e += FFT_T) {
            const int l = e / H, zz = e - l * H;
            const double2 u0 = buf[l * LS + lx<N>(2 * zz)], u1 = buf[l * LS + lx<N>(2 * zz + 1)];
            cm[(row0 + 2 * l) * zpc + zz] = make_double2(u0.x, u1.x);
            cm[(row0 + 2 * l + 1) * zpc + zz] = make_double2(u0.y, u1.y);
        }
        if(!more)
            break;
        __syncthreads();
        t = tn;
    }
#undef FFT_FETCH
}

/* Y and X passes on contiguous tiles.  Tile t = (o, zb), o = t / nzb: N rows of 4 columns at src + t * 4 N.  MODE as in fft_pass_strided,
 * and the fused X pass (MODE 2) split in two for a caller that needs the density spectrum between them (shq_pm_forward):
 *   MODE 3: X forward, the spectrum written back as the contiguous tile it came from (LX, dst = src); with ga.ps the P(k) sums of the
 *           density as the tile is stored.
 *   MODE 4: reads that tile and multiplies every mode by T[k2], then by MODE 2's Green's factor with MODE 2's arithmetic - (v T) green,
 *           potential_transfer's order (gravpm.cpp:412-443) - as it lands in LDS; with ga.ps the P(k) sums of v T; then X inverse.
 *           T = 1 gives MODE 2's bits: v * 1.0 is exact.  T[k2] is fetched with the tile's prefetch.
 *   MODE 5: a sibling of MODE 4 for the excursion-set filters (uvbg.hip): reads that tile, every mode becomes (v / ncell) T[k2] -
 *           divide_by_ncell, then filter_pm (uvbg.cpp:211-250) - with no Green's function, then X inverse.  The kept tile is not written.
 * SCATTER: row i of the result goes to dst + ((i * nzb + zb) * N + o) * 4 (the other layout: a 64-byte piece); otherwise the tile is
 * written back where it came from (dst may be src). */
template <int N, int MODE, bool SCATTER>
__global__ __launch_bounds__(FFT_T, fft_tile_waves(N, MODE)) void fft_t_tile(const double2 *src, double2 *dst, const int nzb, const int ntot,
                                                                       const double2 *__restrict__ W, const GreenArgs ga, const unsigned xcdk)
{
    extern __shared__ double2 buf[];
    constexpr int LS = fft_ls(N);
    constexpr int E = (FFT_C * N + FFT_T - 1) / FFT_T;
    constexpr bool EXACT = E * FFT_T == FFT_C * N;
    double2 *Wl = lds_twiddles<N>(buf, W);
    double *gax = reinterpret_cast<double *>(Wl + fft_twn(N)); /* MODES 2, 4: the Green's function's per-axis factors (fft_gax_kernel) in LDS */
    if(MODE == 2 || MODE == 4) {
        for(int i = threadIdx.x; i < N; i += FFT_T)
            gax[i] = ga.gaxg[i];
        __syncthreads();
    }
    /* MODES 3, 4 with ga.ps: the workgroup's P(k) histogram [3][N] behind the tables, flushed once when the workgroup ends */
    double *hist = MODE == 4 ? gax + N : gax;
    const bool pk = (MODE == 3 || MODE == 4) && ga.ps;
    if(pk) {
        for(int i = threadIdx.x; i < 3 * N; i += FFT_T)
            hist[i] = 0;
        __syncthreads();
    }
    const unsigned vb = xcd_block(blockIdx.x, gridDim.x, xcdk);
    double prx[E], pry[E];
    double tfac[MODE == 4 || MODE == 5 ? E : 1]; /* MODES 4, 5: T[k2] of the prefetched tile's modes */
#define FFT_FETCH(T_)                                                                            \
    {                                                                                            \
        const double2 *b_ = src + (long long) (T_) * (FFT_C * N);                                \
        _Pragma("unroll") for(int i = 0; i < E; i++)                                             \
        {                                                                                        \
            const int e_ = threadIdx.x + i * FFT_T, e = (EXACT || e_ < FFT_C * N) ? e_ : 0; /* no branch around the loads: see fft_t_z_inv */ \
            { \
                const double2 t_ = b_[e];                                                        \
                prx[i] = t_.x;                                                                   \
                pry[i] = t_.y;                                                                   \
            }                                                                                    \
        }                                                                                        \
    }
    /* MODE 4: T[k2] of tile T_'s modes, gathered after the FFT stages (held across them, these registers made the pass spill) so that
     * the scattered stores of the current tile hide the gather.  A pad column (z > N / 2) reads entry 0: k2 stays inside the table */
#define FFT_TFETCH(T_)                                                                           \
    if(MODE == 4 || MODE == 5) {                                                                 \
        const int o_ = (T_) / nzb, zb_ = (T_) - o_ * nzb, y_ = ga.y0 + o_, ky_ = y_ <= N / 2 ? y_ : y_ - N; \
        _Pragma("unroll") for(int i = 0; i < E; i++)                                             \
        {                                                                                        \
            const int e_ = threadIdx.x + i * FFT_T, e = (EXACT || e_ < FFT_C * N) ? e_ : 0;     \
            const int x_ = e / FFT_C, z_ = zb_ * FFT_C + e % FFT_C, kx_ = x_ <= N / 2 ? x_ : x_ - N; \
            const int k2_ = z_ <= N / 2 ? kx_ * kx_ + ky_ * ky_ + z_ * z_ : 0;                   \
            tfac[i] = ga.modefac[k2_ & ga.fac_mask];                                             \
        }                                                                                        \
    }
    int t = (int) vb;
    if(t >= ntot)
        return;
    FFT_FETCH(t)
    FFT_TFETCH(t)
    while(true) {
        const int o = t / nzb, zb = t - o * nzb;
        if(MODE == 4) {
            /* (v T) green: the tile lands multiplied by T, then a rolled sweep over LDS takes its P(k) and applies the fused pass's Green's
             * factor (below) - the factor's division unrolled over the landing took the pass to 190-256 VGPRs */
            const int y = ga.y0 + o, z0 = zb * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N) {
                    const int x = e / FFT_C, z = z0 + e % FFT_C;
                    const int kx = x <= N / 2 ? x : x - N;
                    const double tv = (z <= N / 2 && kx * kx + ky * ky + z * z != 0) ? tfac[i] : 1.0; /* T[0] is not used: the zero mode is removed */
                    buf[(e % FFT_C) * LS + lx<N>(x)] = make_double2(prx[i] * tv, pry[i] * tv);
                }
            }
            __syncthreads();
            const double gy = gax[y] * ga.pot_factor, ky2 = (double) ky * (double) ky;
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T) {
                const int x = e / FFT_C, col = e % FFT_C, z = z0 + col;
                const int kx = x <= N / 2 ? x : x - N;
                double2 *p = buf + col * LS + lx<N>(x);
                const double2 v = *p;
                if(pk)
                    pk_add<N>(hist, ga, v, x, y, z, kx * kx + ky * ky + z * z);
                const double k2 = (double) kx * (double) kx + (ky2 + (double) z * (double) z);
                const double fac = (k2 == 0.0 || z > N / 2) ? 0.0 : gax[x] * gy * gax[z] / k2;
                *p = make_double2(v.x * fac, v.y * fac);
            }
        } else if(MODE == 5) {
            /* value /= total_n_cells, then value *= filter: a division and a multiplication, never contracted */
#pragma clang fp contract(off)
            const double nc = (double) ga.ncell;
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N)
                    buf[(e % FFT_C) * LS + lx<N>(e / FFT_C)] = make_double2((prx[i] / nc) * tfac[i], (pry[i] / nc) * tfac[i]);
            }
        } else {
#pragma unroll
            for(int i = 0; i < E; i++) {
                const int e = threadIdx.x + i * FFT_T;
                if(EXACT || e < FFT_C * N)
                    buf[(e % FFT_C) * LS + lx<N>(e / FFT_C)] = make_double2(prx[i], pry[i]);
            }
        }
        __syncthreads();
        const int tn = t + (int) gridDim.x;
        const bool more = tn < ntot;
        const int tf = more ? tn : t;
        FFT_FETCH(tf)
        if(MODE == 0 || MODE == 3)
            fft_lines<N, -1>(buf, Wl);
        if(MODE == 2) { /* potential_transfer as in fft_pass_strided: line index = kx, o = ky, columns z' = 4 zb .. 4 zb + 3 */
            const int y = ga.y0 + o, z0 = zb * FFT_C;
            const int ky = y <= N / 2 ? y : y - N;
            const double gy = gax[y] * ga.pot_factor, ky2 = (double) ky * (double) ky;
            auto green = [=](int col, int x, double2 v) {
                const int z = z0 + col;
                const int kx = x <= N / 2 ? x : x - N;
                const double k2 = (double) kx * (double) kx + (ky2 + (double) z * (double) z);
                const double fac = (k2 == 0.0 || z > N / 2) ? 0.0 : gax[x] * gy * gax[z] / k2;
                return make_double2(v.x * fac, v.y * fac);
            };
            fft_lines<N, -1>(buf, Wl, green);
            fft_lines<N, +1>(buf, Wl);
        }
        if(MODE == 1 || MODE == 4 || MODE == 5)
            fft_lines<N, +1>(buf, Wl);
        FFT_TFETCH(tf)
        if(MODE == 3) { /* the spectrum back where the tile came from; the density's P(k) on the way */
            double2 *ob = dst + (long long) t * (FFT_C * N);
            const int y = ga.y0 + o;
            const int ky = y <= N / 2 ? y : y - N;
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T) {
                const int x = e / FFT_C, z = zb * FFT_C + e % FFT_C;
                const double2 v = buf[(e % FFT_C) * LS + lx<N>(x)];
                ob[e] = v;
                if(pk) {
                    const int kx = x <= N / 2 ? x : x - N;
                    pk_add<N>(hist, ga, v, x, y, z, kx * kx + ky * ky + z * z);
                }
            }
        } else if(SCATTER) {
            double2 *ob = dst + ((long long) zb * N + o) * FFT_C;
            const long long rs = (long long) nzb * N * FFT_C;
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T) {
                const int row = e / FFT_C, col = e - row * FFT_C;
                ob[(long long) row * rs + col] = buf[col * LS + lx<N>(row)];
            }
        } else {
            double2 *ob = dst + (long long) t * (FFT_C * N);
            for(int e = threadIdx.x; e < FFT_C * N; e += FFT_T)
                ob[e] = buf[(e % FFT_C) * LS + lx<N>(e / FFT_C)];
        }
        if(!more)
            break;
        __syncthreads();
        t = tn;
    }
#undef FFT_FETCH
#undef FFT_TFETCH
    if(pk) { /* one atomic per non-empty bin, as pm_power_kernel */
        __syncthreads();
        unsigned long long *nmodes = reinterpret_cast<unsigned long long *>(ga.ps + 2 * N);
        for(int i = threadIdx.x; i < N; i += FFT_T)
            if(hist[2 * N + i] != 0) {
                atomicAdd(&ga.ps[i], hist[i]);
                atomicAdd(&ga.ps[N + i], hist[N + i]);
                atomicAdd(&nmodes[i], (unsigned long long) hist[2 * N + i]);
            }
    }
}

/* exp(-k_i^2 asmth2) sinctab[i]^2 per mesh index: the expression the in-place X pass fills its LDS table with */
__global__ void fft_gax_kernel(int N, const double *__restrict__ sinctab, double asmth2, double *gax)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < N) {
        const int k = i <= N / 2 ? i : i - N;
        const double sc = sinctab[i];
        gax[i] = exp(-(double) k * (double) k * asmth2) * sc * sc;
    }
}

/* ---- host driver */

/* one kernel at the dynamic LDS size it is launched with */
struct FftKernel {
    const void *fn;
    size_t lds;
    template <class K>
    FftKernel(K *kernel, size_t lds_) : fn((const void *) kernel), lds(lds_)
    {
    }
};

/* The workgroups of `threads` threads resident on `ncu` CUs at once, the least over kernels that share a grid; lifts the 48 KB limit of
 * dynamic LDS on the current device for those that need it.  Without an answer: 1 workgroup per CU. */
int fft_resident(int ncu, int threads, std::initializer_list<FftKernel> kernels, unsigned *res)
{
    *res = ~0u;
    for(const FftKernel &k : kernels) {
        if(k.lds > 48 * 1024)
            SHQ_HIP(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) k.lds));
        int per_cu = 0;
        if(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, threads, k.lds) != hipSuccess || per_cu < 1)
            per_cu = 1;
        const unsigned r = (unsigned) per_cu * (unsigned) ncu;
        *res = r < *res ? r : *res;
    }
    return SHQ_OK;
}

int fft_ncu(const shq_context *ctx)
{
    int ncu = 0;
    if(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || ncu < 1)
        ncu = 256;
    return ncu;
}

/* the context's plan of mesh size N, empty the first time.  The plans of every size used so far stay (uvbg.hip runs a mesh of its own
 * between PM steps of another); a later push_back may move them, so the reference lasts for one call. */
shq_fft_plan &fft_plan(shq_context *ctx, int N)
{
    for(shq_fft_plan &p : ctx->fft_plans)
        if(p.N == N)
            return p;
    ctx->fft_plans.emplace_back();
    ctx->fft_plans.back().N = N;
    return ctx->fft_plans.back();
}

/* The tuning knobs, read on every call (a live process may change them).  Persistent grids: SHQ_FFT_GRID_MUL times the resident
 * workgroups, 0 for one workgroup per tile; SHQ_FFT_XCD_K is fft_pass_strided's and fft_t_tile's xcdk. */
struct FftKnobs {
    unsigned gmul = getenv("SHQ_FFT_GRID_MUL") ? (unsigned) atoi(getenv("SHQ_FFT_GRID_MUL")) : 8u;
    unsigned xcdk = getenv("SHQ_FFT_XCD_K") ? (unsigned) atoi(getenv("SHQ_FFT_XCD_K")) : 8u;
    dim3 grid(int tot, unsigned resident) const
    {
        const unsigned cap = gmul == 0 ? (unsigned) tot : resident * gmul;
        return dim3((unsigned) tot < cap ? (unsigned) tot : cap);
    }
};

/* W: the twiddles of N (ensure_twiddles, or a caller's own); d_out: where T_FILTER's Z inverse writes */
template <int N>
int run_t(shq_context *ctx, const double2 *W, double *d_mesh, double *d_scratch, double *d_out, int zp, bool from_i64, double inv_scale,
          const GreenArgs &ga, shq_fft_part part)
{
    constexpr size_t lds = sizeof(double2) * (FFT_C * fft_ls(N) + fft_twn(N)), lds_x = lds + sizeof(double) * N; /* X pass: + its factor table */
    constexpr size_t lds_hist = sizeof(double) * 3 * N;                                                          /* MODES 3, 4: + the P(k) histogram */
    const int ztot = (int) (((long long) N * N) / (2 * FFT_C));
    const int zpc = zp / 2, nzb = zpc / FFT_C;
    const int stot = N * nzb;
    double2 *A = reinterpret_cast<double2 *>(d_mesh), *B = reinterpret_cast<double2 *>(d_scratch);
    hipStream_t s = ctx->stream;
    auto &pl = fft_plan(ctx, N).t;
    if(pl.res_s == 0) {
        auto p = pl;
        const int ncu = fft_ncu(ctx);
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_t_z_fwd<N, true>, lds}, {fft_t_z_fwd<N, false>, lds}, {fft_t_z_inv<N>, lds}}, &p.res_z));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_t_tile<N, 2, true>, lds_x}}, &p.res_x));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_t_tile<N, 3, false>, lds + lds_hist}}, &p.res_x3));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_t_tile<N, 4, true>, lds_x + lds_hist}}, &p.res_x4));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_t_tile<N, 5, true>, lds}}, &p.res_x5));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_t_tile<N, 0, true>, lds}, {fft_t_tile<N, 1, false>, lds}}, &p.res_s));
        pl = p;
    }
    const FftKnobs k{};
    const unsigned xcdk = k.xcdk;
    const dim3 gz = k.grid(ztot, pl.res_z), gs = k.grid(stot, pl.res_s), gx = k.grid(stot, pl.res_x);
    if(part == SHQ_FFT_T_SOLVE || part == SHQ_FFT_T_FORWARD) {
        if(from_i64)
            fft_t_z_fwd<N, true><<<gz, dim3(FFT_T), lds, s>>>(d_mesh, B, ztot, zp, W, inv_scale);
        else
            fft_t_z_fwd<N, false><<<gz, dim3(FFT_T), lds, s>>>(d_mesh, B, ztot, zp, W, 1.0);
        fft_t_tile<N, 0, true><<<gs, dim3(FFT_T), lds, s>>>(B, A, nzb, stot, W, ga, xcdk);
    }
    if(part == SHQ_FFT_T_SOLVE)
        fft_t_tile<N, 2, true><<<gx, dim3(FFT_T), lds_x, s>>>(A, B, nzb, stot, W, ga, xcdk);
    else if(part == SHQ_FFT_T_FORWARD)
        fft_t_tile<N, 3, false><<<k.grid(stot, pl.res_x3), dim3(FFT_T), lds + (ga.ps ? lds_hist : 0), s>>>(A, A, nzb, stot, W, ga, xcdk);
    else if(part == SHQ_FFT_T_FINISH)
        fft_t_tile<N, 4, true><<<k.grid(stot, pl.res_x4), dim3(FFT_T), lds_x + (ga.ps ? lds_hist : 0), s>>>(A, B, nzb, stot, W, ga, xcdk);
    else
        fft_t_tile<N, 5, true><<<k.grid(stot, pl.res_x5), dim3(FFT_T), lds, s>>>(A, B, nzb, stot, W, ga, xcdk);
    if(part != SHQ_FFT_T_FORWARD) {
        fft_t_tile<N, 1, false><<<gs, dim3(FFT_T), lds, s>>>(B, B, nzb, stot, W, ga, xcdk);
        fft_t_z_inv<N><<<gz, dim3(FFT_T), lds, s>>>(B, part == SHQ_FFT_T_FILTER ? d_out : d_mesh, ztot, zp, W);
    }
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* nslab: N for the stages of a full cube */
template <int N>
int run_n(shq_context *ctx, const double2 *W, double *d_mesh, int zp, shq_fft_stage stage, bool from_i64, double inv_scale, const GreenArgs &ga,
          int nslab)
{
    /* FFT_C padded lines + the twiddle table + (X pass) the sinc table */
    constexpr size_t lds = sizeof(double2) * (FFT_C * fft_ls(N) + fft_twn(N)) + sizeof(double) * N;
    constexpr size_t lds_hist = lds + sizeof(double) * 3 * N; /* the split X pass with the P(k) histogram */
#ifndef SHQ_FFT_RELAX /* tile-shape experiments on one mesh size */
    static_assert(N % (2 * FFT_C) == 0, "rows must tile evenly");
#endif
    const int ztot = (int) (((long long) nslab * N) / (2 * FFT_C)); /* row groups of the Z passes */
    const int zpc = zp / 2;
    const int ntiles = zpc / FFT_C;
    const int stot = nslab * ntiles;                                  /* tiles of a strided pass */
    double2 *cm = reinterpret_cast<double2 *>(d_mesh);
    hipStream_t s = ctx->stream;
    /* persistent grids: as many workgroups as are resident on the chip at once (LDS-limited); the split X pass has counts of its own
     * (as fft_t_tile's res_x3 / res_x4), so that the histogram's LDS does not shrink the grids of the other passes */
    auto &pl = fft_plan(ctx, N).n;
    if(pl.res_s == 0) {
        auto p = pl;
        const int ncu = fft_ncu(ctx);
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_z_fwd<N, true>, lds}, {fft_pass_z_fwd<N, false>, lds}}, &p.res_zf));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_z_inv<N>, lds}}, &p.res_zi));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_strided<N, 3>, lds_hist}}, &p.res_x3));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_strided<N, 4>, lds_hist}}, &p.res_x4));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_strided<N, 5>, lds}}, &p.res_x5));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_strided<N, 6>, lds}}, &p.res_x6));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_strided<N, 7>, lds_hist}}, &p.res_x7));
        SHQ_TRY(fft_resident(ncu, FFT_T, {{fft_pass_strided<N, 8>, lds}}, &p.res_x8));
        SHQ_TRY(fft_resident(ncu, FFT_T,
                             {{fft_pass_strided<N, 0>, lds}, {fft_pass_strided<N, 1>, lds}, {fft_pass_strided<N, 2>, lds}, {fft_pass_strided<N, 0, 1>, lds},
                              {fft_pass_strided<N, 1, 2>, lds}},
                             &p.res_s));
        pl = p;
    }
    const FftKnobs k{};
    const unsigned xcdk = k.xcdk;
    const dim3 gzf = k.grid(ztot, pl.res_zf), gzi = k.grid(ztot, pl.res_zi), gs = k.grid(stot, pl.res_s);
    auto z_forward = [&] {
        if(from_i64)
            fft_pass_z_fwd<N, true><<<gzf, dim3(FFT_T), lds, s>>>(d_mesh, ztot, zp, W, inv_scale);
        else
            fft_pass_z_fwd<N, false><<<gzf, dim3(FFT_T), lds, s>>>(d_mesh, ztot, zp, W, 1.0);
    };
    const bool packed = stage == SHQ_FFT_YZ_FORWARD_PACKED || stage == SHQ_FFT_YZ_INVERSE_PACKED; /* the Y pass's other side is ga.alt */
    const size_t lds_split = ga.ps ? lds_hist : lds;
    switch(stage) {
    case SHQ_FFT_X_SOLVE: /* lines along x of a y-slab: element stride nslab * zpc, outer = local y */
        fft_pass_strided<N, 2><<<gs, dim3(FFT_T), lds, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_X_FORWARD_SUMS:
        fft_pass_strided<N, 3><<<k.grid(stot, pl.res_x3), dim3(FFT_T), lds_split, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_X_FINISH:
        fft_pass_strided<N, 4><<<k.grid(stot, pl.res_x4), dim3(FFT_T), lds_split, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_X_FILTER:
        fft_pass_strided<N, 5><<<k.grid(stot, pl.res_x5), dim3(FFT_T), lds, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_X_ZEL:
        fft_pass_strided<N, 6><<<k.grid(stot, pl.res_x6), dim3(FFT_T), lds, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_X_GLASS_FORWARD:
        fft_pass_strided<N, 7><<<k.grid(stot, pl.res_x7), dim3(FFT_T), lds_split, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_X_GLASS:
        fft_pass_strided<N, 8><<<k.grid(stot, pl.res_x8), dim3(FFT_T), lds, s>>>(cm, (long long) nslab * zpc, zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_YZ_FORWARD:
    case SHQ_FFT_YZ_FORWARD_PACKED:
        z_forward();
        if(packed)
            fft_pass_strided<N, 0, 1><<<gs, dim3(FFT_T), lds, s>>>(cm, zpc, (long long) N * zpc, ntiles, stot, W, ga, xcdk);
        else
            fft_pass_strided<N, 0><<<gs, dim3(FFT_T), lds, s>>>(cm, zpc, (long long) N * zpc, ntiles, stot, W, ga, xcdk);
        break;
    case SHQ_FFT_YZ_INVERSE:
    case SHQ_FFT_YZ_INVERSE_PACKED:
        if(packed)
            fft_pass_strided<N, 1, 2><<<gs, dim3(FFT_T), lds, s>>>(cm, zpc, (long long) N * zpc, ntiles, stot, W, ga, xcdk);
        else
            fft_pass_strided<N, 1><<<gs, dim3(FFT_T), lds, s>>>(cm, zpc, (long long) N * zpc, ntiles, stot, W, ga, xcdk);
        fft_pass_z_inv<N><<<gzi, dim3(FFT_T), lds, s>>>(d_mesh, ztot, zp, W);
        break;
    case SHQ_FFT_FORWARD:
    case SHQ_FFT_INVERSE:
    case SHQ_FFT_SOLVE:
        if(stage != SHQ_FFT_INVERSE) {
            z_forward();
            /* Y: outer = x plane (stride N*zpc), element stride zpc */
            fft_pass_strided<N, 0><<<gs, dim3(FFT_T), lds, s>>>(cm, zpc, (long long) N * zpc, ntiles, stot, W, ga, xcdk);
        }
        /* X: outer = y (stride zpc), element stride N*zpc */
        if(stage == SHQ_FFT_FORWARD)
            fft_pass_strided<N, 0><<<gs, dim3(FFT_T), lds, s>>>(cm, (long long) N * zpc, zpc, ntiles, stot, W, ga, xcdk);
        else if(stage == SHQ_FFT_INVERSE)
            fft_pass_strided<N, 1><<<gs, dim3(FFT_T), lds, s>>>(cm, (long long) N * zpc, zpc, ntiles, stot, W, ga, xcdk);
        else
            fft_pass_strided<N, 2><<<gs, dim3(FFT_T), lds, s>>>(cm, (long long) N * zpc, zpc, ntiles, stot, W, ga, xcdk);
        if(stage != SHQ_FFT_FORWARD) {
            fft_pass_strided<N, 1><<<gs, dim3(FFT_T), lds, s>>>(cm, zpc, (long long) N * zpc, ntiles, stot, W, ga, xcdk);
            fft_pass_z_inv<N><<<gzi, dim3(FFT_T), lds, s>>>(d_mesh, ztot, zp, W);
        }
        break;
    }
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* mesh sizes with a compiled pipeline (multiples of 8 of the form 2^a 3^b 5^c) */
#define SHQ_FFT_SIZES(X) \
    X(16) X(24) X(32) X(40) X(48) X(64) X(80) X(96) X(128) X(192) X(256) X(384) X(512) X(768) X(960) X(1024) X(1152) X(1200) X(1536)

template <int NN>
struct FftSize {
    enum { N = NN };
};

/* f(FftSize<N>()) for a compiled N */
template <class F>
int fft_dispatch(int N, F f)
{
    switch(N) {
#define SHQ_FFT_CASE(NN) \
    case NN: return f(FftSize<NN>());
        SHQ_FFT_SIZES(SHQ_FFT_CASE)
#undef SHQ_FFT_CASE
    }
    return SHQ_ERR_INVALID;
}

int ensure_twiddles(shq_context *ctx, int N)
{
    if(ctx->fft_tw_n == N)
        return SHQ_OK;
    SHQ_TRY(ctx->fft_tw.reserve(2 * (size_t) N));
    SHQ_TRY(shq_fft3d_fill_twiddles(N, ctx->fft_tw.ptr));
    ctx->fft_tw_n = N;
    return SHQ_OK;
}

} // namespace

bool shq_fft3d_supported(int N)
{
    switch(N) {
#define SHQ_FFT_CASE(NN) case NN:
        SHQ_FFT_SIZES(SHQ_FFT_CASE)
#undef SHQ_FFT_CASE
        return true;
    }
    return false;
}

/* z pitch (in doubles) the bespoke pipeline wants: N/2+1 complex rounded up to a multiple of the tile width FFT_C (4). */
int shq_fft3d_pitch(int N) { return 2 * (((N / 2 + 1) + FFT_C - 1) / FFT_C * FFT_C); }

/* the N twiddles exp(-2 pi i k / N) as (re, im) into a device table of 2 N doubles */
int shq_fft3d_fill_twiddles(int N, double *d_tw)
{
    std::vector<double> h(2 * (size_t) N);
    for(int k = 0; k < N; k++) {
        h[2 * k] = cos(2 * M_PI * k / N);
        h[2 * k + 1] = -sin(2 * M_PI * k / N);
    }
    SHQ_HIP(hipMemcpy(d_tw, h.data(), sizeof(double) * 2 * N, hipMemcpyHostToDevice));
    return SHQ_OK;
}

/* The transposing pipeline: d_scratch is a second mesh of the same size.  The excursion-set radius loop (uvbg.hip) passes twiddles of
 * its own and no sinc table, and so touches none of the context's FFT tables (its twiddles, the Green's factor table). */
int shq_fft3d_run_transposed(shq_context *ctx, double *d_mesh, double *d_scratch, int N, int zp, shq_fft_part part, bool from_i64, double inv_scale,
                             const double *d_sinctab, double asmth2, double pot_factor, const shq_fft_opts &o)
{
    if(part == SHQ_FFT_T_FILTER)
        SHQ_CHECK(o.modefac && o.out && o.out != d_mesh && o.out != d_scratch && o.tw && o.ncell > 0, SHQ_ERR_INVALID,
                  "fft3d: bad filter part arguments");
    else
        SHQ_CHECK(part >= SHQ_FFT_T_SOLVE && part <= SHQ_FFT_T_FINISH && (part != SHQ_FFT_T_FINISH || o.modefac) && (!o.ps || o.bintab),
                  SHQ_ERR_INVALID, "fft3d: bad part arguments");
    SHQ_CHECK(shq_fft3d_supported(N) && N % (2 * FFT_C) == 0, SHQ_ERR_INVALID, "fft3d: unsupported mesh size %d", N);
    SHQ_CHECK(zp == shq_fft3d_pitch(N) && d_mesh && d_scratch && d_mesh != d_scratch, SHQ_ERR_INVALID, "fft3d: bad pitch or scratch mesh");
    if(!o.tw)
        SHQ_TRY(ensure_twiddles(ctx, N));
    GreenArgs ga;
    ga.sinctab = d_sinctab;
    ga.asmth2 = asmth2;
    ga.pot_factor = pot_factor;
    ga.modefac = o.modefac;
    ga.fac_mask = o.fac_mask;
    ga.bintab = o.bintab;
    ga.ps = o.ps;
    ga.ncell = o.ncell;
    if(d_sinctab) {
        if(ctx->fft_gax_n != N || ctx->fft_gax_asmth2 != asmth2 || ctx->fft_gax_src != d_sinctab) {
            SHQ_TRY(ctx->fft_gax.reserve((size_t) N));
            fft_gax_kernel<<<dim3((unsigned) ((N + 255) / 256)), dim3(256), 0, ctx->stream>>>(N, d_sinctab, asmth2, ctx->fft_gax.ptr);
            SHQ_HIP(hipGetLastError());
            ctx->fft_gax_n = N;
            ctx->fft_gax_asmth2 = asmth2;
            ctx->fft_gax_src = d_sinctab;
        }
        ga.gaxg = ctx->fft_gax.ptr;
    }
    const double2 *W = reinterpret_cast<const double2 *>(o.tw ? o.tw : ctx->fft_tw.ptr);
    return fft_dispatch(N, [&](auto n) { return run_t<decltype(n)::N>(ctx, W, d_mesh, d_scratch, o.out, zp, from_i64, inv_scale, ga, part); });
}

/* The in-place pipeline on d_mesh = [N][N][zp] doubles, or on a rank's slab of it */
int shq_fft3d_run(shq_context *ctx, double *d_mesh, int N, int zp, shq_fft_stage stage, bool from_i64, double inv_scale, const double *d_sinctab,
                  double asmth2, double pot_factor, const shq_fft_opts &o)
{
    const bool yslab = stage == SHQ_FFT_X_SOLVE || stage == SHQ_FFT_X_FORWARD_SUMS || stage == SHQ_FFT_X_FINISH || stage == SHQ_FFT_X_FILTER ||
                       stage == SHQ_FFT_X_ZEL || stage == SHQ_FFT_X_GLASS_FORWARD || stage == SHQ_FFT_X_GLASS;
    const bool packed = stage == SHQ_FFT_YZ_FORWARD_PACKED || stage == SHQ_FFT_YZ_INVERSE_PACKED;
    const int nslab = stage <= SHQ_FFT_SOLVE ? N : o.nslab;
    SHQ_CHECK(shq_fft3d_supported(N), SHQ_ERR_INVALID, "fft3d: unsupported mesh size %d", N);
    SHQ_CHECK(nslab > 0 && nslab <= N && o.y0 >= 0 && o.y0 + (yslab ? nslab : 0) <= N, SHQ_ERR_INVALID, "fft3d: bad slab geometry");
    SHQ_CHECK(zp >= N + 2 && zp % 8 == 0, SHQ_ERR_INVALID, "fft3d: pitch %d must be a multiple of 8 doubles and >= N+2", zp);
    SHQ_CHECK((stage != SHQ_FFT_X_FINISH || o.modefac) && (!o.ps || o.bintab), SHQ_ERR_INVALID, "fft3d: bad split X pass arguments");
    SHQ_CHECK(stage != SHQ_FFT_X_FILTER || (o.modefac && o.out && o.out != d_mesh && o.ncell > 0), SHQ_ERR_INVALID,
              "fft3d: bad filter pass arguments");
    SHQ_CHECK(stage != SHQ_FFT_X_ZEL || (o.modefac && o.fac_mask == -1 && o.out && o.out != d_mesh && o.zel_axis >= -1 && o.zel_axis <= 2),
              SHQ_ERR_INVALID, "fft3d: bad transfer pass arguments");
    SHQ_CHECK(stage != SHQ_FFT_X_GLASS_FORWARD || !o.ps || d_sinctab, SHQ_ERR_INVALID, "fft3d: the glass's sums need the sinc table");
    SHQ_CHECK(stage != SHQ_FFT_X_GLASS || (o.modefac && o.out && o.out != d_mesh && o.zel_axis >= 0 && o.zel_axis <= 2), SHQ_ERR_INVALID,
              "fft3d: bad glass transfer pass arguments");
    if(!o.tw)
        SHQ_TRY(ensure_twiddles(ctx, N));
    GreenArgs ga;
    ga.sinctab = d_sinctab;
    ga.asmth2 = asmth2;
    ga.pot_factor = pot_factor;
    ga.zel_axis = o.zel_axis;
    ga.zel_c0 = o.zel_c0;
    ga.y0 = o.y0;
    ga.alt = reinterpret_cast<double2 *>(o.packed);
    ga.modefac = o.modefac;
    ga.fac_mask = o.fac_mask;
    ga.bintab = o.bintab;
    ga.ps = o.ps;
    ga.ncell = o.ncell;
    ga.out = reinterpret_cast<double2 *>(o.out);
    if(packed) {
        SHQ_CHECK(o.packed && o.nranks >= 1 && N % o.nranks == 0, SHQ_ERR_INVALID,
                  "fft3d: packed stages need a buffer and a rank count that divides the mesh");
        ga.nyl = N / o.nranks;
        ga.alt_outer = (long long) ga.nyl * (zp / 2);
        ga.qstride = (long long) nslab * ga.alt_outer;
    }
    const double2 *W = reinterpret_cast<const double2 *>(o.tw ? o.tw : ctx->fft_tw.ptr);
    return fft_dispatch(N, [&](auto n) { return run_n<decltype(n)::N>(ctx, W, d_mesh, zp, stage, from_i64, inv_scale, ga, nslab); });
}
