/* thermal.hip — the thermal velocities of warm dark matter and neutrino particles on the device for one rank: add_thermal_speeds
 * (libgenic/thermal.cpp:95-110) in the particle loops of genic/main.cpp:176-184 and 218-226, with init_rng (thermal.cpp:77-91) and
 * init_thermalvel's tables (thermal.cpp:44-75) on the host.
 *
 * The reference runs one serial loop: a boost::random::ranlux48 reseeded at the start of every grid column (x, y), three draws per
 * particle along z.  ranlux48 keeps 11 of every 389 steps of a 48-bit subtract-with-carry recurrence with lags 5 and 12, so a draw costs
 * about 35 dependent steps; the columns are independent, so thermal_speeds_kernel runs ONE engine per lane.
 *  - The 12 state words and the carry live in registers.  A step at word k reads word k - 5, so a block of 389 steps is written with
 *    compile-time word positions: 11 kept steps at words 0..10, then the 378 dropped ones as word 11, 31 whole rounds of 12 and words
 *    0..4.  389 = 5 mod 12: the next block would start at word 5, so the words are renamed by 5 (x[j] <- x[j + 5]) and every block is the
 *    same code.  The 11 kept outputs ARE words 0..10 until the dropped steps run, so the dropped steps run lazily, before the 12th draw;
 *    a draw picks its word with a chain of selects on compile-time indices.  Nothing is indexed at run time, and the code object's
 *    metadata shows no private segment.
 *  - A wave works on 64 columns x TZ particles at a time.  The columns are Ngrid * 12 bytes apart in vel, so the tile goes through LDS:
 *    read as runs of TZ * 12 contiguous bytes per column, updated by the lane that owns the column, written back the same way.
 *  - The bin of p is found by a binary search over the 2000 cumprob knots.  Knots, speeds and slopes (48 KB) are left to the caches: a
 *    copy of the knots in LDS (16 KB per one-wave workgroup) measured 8 % faster at Ngrid = 256, where every wave is resident either
 *    way, and 53 % slower at 512, where it is LDS that then limits the waves per CU, and was not kept.
 * The two readings of boost that this file rests on (the engine and the makima evaluation) are stated in shenqi_hip.h.
 * The call owns every buffer it uses and changes nothing of the context but its phase times.
 */
#include "call_scope.hpp"
#include "makima.hpp" /* makima_slopes */
#include <math.h>
#include <string.h>
#include <random>
#include <vector>

namespace {

constexpr int TW = 64;                /* one wave per workgroup, one column per lane */
constexpr int TZ = 16;                /* particles per column in one LDS tile: runs of 192 bytes along z */
constexpr int TRUN = TZ * 3;          /* floats of one column in a tile */
constexpr int NK = SHQ_THERMAL_NKNOTS;
constexpr uint64_t M48 = (1ull << 48) - 1;
constexpr double TWO_M48 = 1.0 / 281474976710656.0; /* 2^-48 */

/* ranlux48 = discard_block<subtract_with_carry<48, 5, 12>, 389, 11>; the position is always word 0 at the start of a block */
struct Ranlux48 {
    uint64_t x[12];
    uint64_t c; /* the carry */
    int n;      /* outputs of this block already handed out; they are x[0..10] */
};

/* y = x[k - 5] - x[k] - carry mod 2^48, the carry set on borrow: both words are below 2^48, so a borrow shows in bit 63 */
#define RL_STEP(g, k)                                                                          \
    do {                                                                                       \
        const uint64_t t_ = (g).x[((k) + 7) % 12] - (g).x[(k)] - (g).c;                        \
        (g).c = t_ >> 63;                                                                      \
        (g).x[(k)] = t_ & M48;                                                                 \
    } while(0)

__device__ __forceinline__ void rl_kept(Ranlux48 &g)
{
#pragma unroll
    for(int k = 0; k < 11; k++)
        RL_STEP(g, k);
    g.n = 0;
}

/* the 378 dropped steps of a block, and the renaming that puts the next block's first word at 0 */
__device__ __forceinline__ void rl_dropped(Ranlux48 &g)
{
    RL_STEP(g, 11);
#pragma unroll 1
    for(int r = 0; r < 31; r++) {
#pragma unroll
        for(int k = 0; k < 12; k++)
            RL_STEP(g, k);
    }
#pragma unroll
    for(int k = 0; k < 5; k++)
        RL_STEP(g, k);
    uint64_t y[12];
#pragma unroll
    for(int k = 0; k < 12; k++)
        y[k] = g.x[(k + 5) % 12];
#pragma unroll
    for(int k = 0; k < 12; k++)
        g.x[k] = y[k];
}

/* seed(v) of a 32-bit value: the LCG 40014 x mod 2147483563 from v mod 2147483563 (1 if that is 0; 19780503 for v == 0), two outputs per
 * word, lo + (hi << 32) mod 2^48; carry = (word[11] == 0) */
__device__ __forceinline__ void rl_seed(Ranlux48 &g, uint32_t v)
{
    uint64_t s = v == 0 ? 19780503u : v;
    s %= 2147483563ull;
    if(s == 0)
        s = 1;
#pragma unroll
    for(int k = 0; k < 12; k++) {
        s = s * 40014ull % 2147483563ull;
        const uint64_t lo = s;
        s = s * 40014ull % 2147483563ull;
        g.x[k] = (lo + (s << 32)) & M48;
    }
    g.c = g.x[11] == 0 ? 1 : 0;
    rl_kept(g);
}

__device__ __forceinline__ uint64_t rl_next(Ranlux48 &g)
{
    if(g.n == 11) { /* the same in every lane of the wave */
        rl_dropped(g);
        rl_kept(g);
    }
    uint64_t r = g.x[0];
#pragma unroll
    for(int k = 1; k < 11; k++)
        r = g.n == k ? g.x[k] : r;
    g.n++;
    return r;
}

/* shq_thermal_column_draws: the first m outputs of engine t */
__global__ __launch_bounds__(TW) void thermal_draws_kernel(int n, const uint32_t *__restrict__ seeds, int m, uint64_t *__restrict__ raw)
{
    const int t = blockIdx.x * TW + threadIdx.x;
    if(t >= n)
        return;
    Ranlux48 g;
    rl_seed(g, seeds[t]);
    for(int q = 0; q < m; q++)
        raw[(size_t) t * m + q] = rl_next(g);
}

/* tab = [cumprob | fdvel | slopes], NK doubles each.  Column c of the rank's sub-block (c = xl * ny + yl) owns the particles
 * [c * N, (c + 1) * N); seeds[c] is its entry of the seed table.  dvel and speed may be null. */
__global__ __launch_bounds__(TW) void thermal_speeds_kernel(int N, int ncol, double v_amp, const uint32_t *__restrict__ seeds,
                                                            const double *__restrict__ tab, float *__restrict__ vel,
                                                            double *__restrict__ dvel, double *__restrict__ speed)
{
#pragma clang fp contract(off)
    __shared__ float tile[TW][TRUN + 1];
    const int lane = threadIdx.x;
    const int cbase = blockIdx.x * TW;
    const int c = cbase + lane;
    const bool act = c < ncol;
    const int ncolw = min(TW, ncol - cbase); /* columns of this wave */
    const double *__restrict__ knots = tab, *__restrict__ fdv = tab + NK, *__restrict__ slope = tab + 2 * NK;
    Ranlux48 g;
    if(act)
        rl_seed(g, seeds[c]);
    for(int z0 = 0; z0 < N; z0 += TZ) {
        const int nz = min(TZ, N - z0), run = nz * 3, total = ncolw * run;
        /* flat index f = col * run + e of the tile, 64 consecutive ones per pass: lanes follow each other along a column's run */
        for(int f = lane, col = 0, e = lane; f < total; f += TW, e += TW) {
            while(e >= run) {
                e -= run;
                col++;
            }
            tile[col][e] = vel[((size_t) (cbase + col) * N + z0) * 3 + e];
        }
        __syncthreads();
        if(act)
            for(int zz = 0; zz < nz; zz++) {
                const double p = (double) rl_next(g) * TWO_M48;
                int lo = 0, hi = NK - 1; /* knots[0] = 0 <= p < 1 = knots[NK - 1] */
                while(hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if(knots[mid] <= p)
                        lo = mid;
                    else
                        hi = mid;
                }
                const double x0 = knots[lo], x1 = knots[lo + 1], y0 = fdv[lo], y1 = fdv[lo + 1], s0 = slope[lo], s1 = slope[lo + 1];
                const double dx = x1 - x0, d = p - x0, t = d / dx, omt = 1 - t;
                const double a = y0 * (1 + 2 * t) + s0 * d;
                const double b = y1 * (3 - 2 * t) + (dx * s1) * (t - 1);
                const double F = (omt * omt) * a + (t * t) * b;
                const double v = v_amp * F;
                const double phi = (2 * M_PI) * ((double) rl_next(g) * TWO_M48);
                const double theta = acos(2 * ((double) rl_next(g) * TWO_M48) - 1);
                double st, ct, sp, cp;
                sincos(theta, &st, &ct);
                sincos(phi, &sp, &cp);
                const double vs = v * st;
                const double inc[3] = {vs * cp, vs * sp, v * ct};
                const size_t ip = (size_t) c * N + z0 + zz;
#pragma unroll
                for(int k = 0; k < 3; k++) {
                    tile[lane][3 * zz + k] = (float) ((double) tile[lane][3 * zz + k] + inc[k]);
                    if(dvel)
                        dvel[3 * ip + k] = inc[k];
                }
                if(speed)
                    speed[ip] = v;
            }
        __syncthreads();
        for(int f = lane, col = 0, e = lane; f < total; f += TW, e += TW) {
            while(e >= run) {
                e -= run;
                col++;
            }
            vel[((size_t) (cbase + col) * N + z0) * 3 + e] = tile[col][e];
        }
        __syncthreads();
    }
}

/* the integral of x^2 / (e^x + 1) over [a, b] by panels of 8-point Gauss-Legendre no wider than 1/64 */
long double fd_integral(double a, double b)
{
    static const long double gx[4] = {0.1834346424956498049394761L, 0.5255324099163289858177390L, 0.7966664774136267395915539L,
                                      0.9602898564975362316835609L};
    static const long double gw[4] = {0.3626837833783619829651504L, 0.3137066458778872873379622L, 0.2223810344533744705443560L,
                                      0.1012285362903762591525314L};
    auto f = [](long double x) { return x * x / (expl(x) + 1); };
    const int np = (int) fmin(1e6, ceil((b - a) * 64)) + 1;
    long double sum = 0;
    for(int q = 0; q < np; q++) {
        const long double lo = a + ((long double) b - a) * q / np, hi = a + ((long double) b - a) * (q + 1) / np;
        const long double mid = (lo + hi) / 2, half = (hi - lo) / 2;
        long double acc = 0;
        for(int k = 0; k < 4; k++)
            acc += gw[k] * (f(mid - half * gx[k]) + f(mid + half * gx[k]));
        sum += acc * half;
    }
    return sum;
}

} // namespace

/* ---- C-ABI ------------------------------------------------------------------------------ */

extern "C" int shq_thermal_seed_table(int Seed, int Ngrid, uint32_t *table)
{
    SHQ_CHECK(table && Ngrid >= 1 && Ngrid <= 46340, SHQ_ERR_INVALID, "thermal_seed_table: null table or Ngrid %d outside [1, 46340]", Ngrid);
    std::ranlux48 rng((uint32_t) Seed); /* boost seeds through a 32-bit cast */
    for(int i = 0; i < Ngrid; i++)
        for(int j = 0; j < Ngrid; j++)
            table[i + (size_t) Ngrid * j] = (uint32_t) rng();
    return SHQ_OK;
}

extern "C" int shq_thermal_tables(double max_fd, double min_fd, double *vel, double *cumprob, double *total_frac)
{
#pragma clang fp contract(off)
    SHQ_CHECK(vel && cumprob && total_frac, SHQ_ERR_INVALID, "thermal_tables: null argument");
    SHQ_CHECK(isfinite(max_fd) && isfinite(min_fd) && max_fd > min_fd, SHQ_ERR_INVALID,
              "thermal_tables: the interval [%g, %g] is empty or not finite", min_fd, max_fd);
    if(max_fd > 17.0) /* MAX_FERMI_DIRAC */
        max_fd = 17.0;
    SHQ_CHECK(max_fd > min_fd, SHQ_ERR_INVALID, "thermal_tables: min_fd %g is not below MAX_FERMI_DIRAC = 17", min_fd);
    std::vector<long double> cum(NK);
    cum[0] = 0;
    for(int i = 0; i < NK; i++)
        vel[i] = min_fd + (max_fd - min_fd) * i / (NK - 1.0);
    for(int i = 1; i < NK; i++)
        cum[i] = cum[i - 1] + fd_integral(vel[i - 1], vel[i]);
    const long double total_fd = fd_integral(0.0, 17.0);
    *total_frac = (double) (cum[NK - 1] / total_fd);
    for(int i = 0; i < NK; i++)
        cumprob[i] = (double) (cum[i] / cum[NK - 1]);
    return SHQ_OK;
}

extern "C" int shq_thermal_phase_ms(shq_context *ctx, double ms[3])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 3; i++)
        ms[i] = ctx->thermal_ms[i];
    return SHQ_OK;
}

extern "C" int shq_thermal_column_draws(shq_context *ctx, int n, const uint32_t *seeds, int m, uint64_t *raw)
{
    SHQ_CHECK(ctx && seeds && raw, SHQ_ERR_INVALID, "thermal: null argument");
    SHQ_CHECK(n >= 1 && n <= 65536 && m >= 1 && m <= (1 << 20), SHQ_ERR_INVALID, "thermal_column_draws: n %d, m %d", n, m);
    SHQ_HIP(hipSetDevice(ctx->device));
    CallScope sc(ctx, "thermal");
    uint32_t *d_seeds;
    uint64_t *d_raw;
    SHQ_TRY(sc.alloc(&d_seeds, (size_t) n));
    SHQ_TRY(sc.alloc(&d_raw, (size_t) n * m));
    hipStream_t s = ctx->stream;
    SHQ_HIP(hipMemcpyAsync(d_seeds, seeds, sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    thermal_draws_kernel<<<dim3(nblk(n, TW)), dim3(TW), 0, s>>>(n, d_seeds, m, d_raw);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(raw, d_raw, sizeof(uint64_t) * n * m, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    return SHQ_OK;
}

extern "C" int shq_thermal_speeds(shq_context *ctx, const shq_thermal_params *p, const uint32_t *seedtable, const double *cumprob,
                                  const double *fdvel, int64_t n, float *vel, double *dvel, double *speed)
{
    SHQ_CHECK(ctx && p && seedtable && cumprob && fdvel && vel, SHQ_ERR_INVALID, "thermal: null argument");
    /* ---- every check before anything is written */
    const int N = p->Ngrid;
    SHQ_CHECK(N >= 2 && N <= 46340, SHQ_ERR_INVALID, "thermal: Ngrid %d outside [2, 46340]", N);
    SHQ_CHECK(p->x0 >= 0 && p->nx >= 1 && p->nx <= N - p->x0 && p->y0 >= 0 && p->ny >= 1 && p->ny <= N - p->y0, SHQ_ERR_INVALID,
              "thermal: the sub-block x [%d, +%d) y [%d, +%d) is not inside the %d^2 grid", p->x0, p->nx, p->y0, p->ny, N);
    const long long ncol = (long long) p->nx * p->ny;
    SHQ_CHECK(n == ncol * N && n < (1ll << 31), SHQ_ERR_INVALID, "thermal: %lld particles, the sub-block holds %lld (< 2^31 on one rank)",
              (long long) n, ncol * N);
    SHQ_CHECK(isfinite(p->v_amp), SHQ_ERR_INVALID, "thermal: v_amp is not finite");
    for(int i = 0; i < NK; i++)
        SHQ_CHECK(isfinite(cumprob[i]) && isfinite(fdvel[i]), SHQ_ERR_INVALID, "thermal: non-finite table entry at knot %d", i);
    SHQ_CHECK(cumprob[0] == 0 && cumprob[NK - 1] == 1, SHQ_ERR_INVALID, "thermal: cumprob runs from %g to %g, not from 0 to 1", cumprob[0],
              cumprob[NK - 1]);
    for(int i = 1; i < NK; i++)
        SHQ_CHECK(cumprob[i] > cumprob[i - 1] && fdvel[i] > fdvel[i - 1], SHQ_ERR_INVALID, "thermal: the tables do not increase strictly at knot %d", i);
    SHQ_HIP(hipSetDevice(ctx->device));
    for(int i = 0; i < 3; i++)
        ctx->thermal_ms[i] = 0;

    /* ---- the columns' seeds (the reference's transposed table read as it is) and [cumprob | fdvel | slopes] */
    std::vector<uint32_t> seeds((size_t) ncol);
    for(int xl = 0; xl < p->nx; xl++)
        for(int yl = 0; yl < p->ny; yl++)
            seeds[(size_t) xl * p->ny + yl] = seedtable[(size_t) (xl + p->x0) * N + (yl + p->y0)];
    std::vector<double> tab((size_t) 3 * NK);
    memcpy(tab.data(), cumprob, sizeof(double) * NK);
    memcpy(tab.data() + NK, fdvel, sizeof(double) * NK);
    makima_slopes(NK, cumprob, fdvel, tab.data() + 2 * NK);

    hipStream_t s = ctx->stream;
    CallScope sc(ctx, "thermal");
    uint32_t *d_seeds;
    double *d_tab, *d_dvel = nullptr, *d_speed = nullptr;
    float *d_vel;
    SHQ_TRY(sc.alloc(&d_seeds, (size_t) ncol));
    SHQ_TRY(sc.alloc(&d_tab, (size_t) 3 * NK));
    SHQ_TRY(sc.alloc(&d_vel, (size_t) 3 * n));
    if(dvel)
        SHQ_TRY(sc.alloc(&d_dvel, (size_t) 3 * n));
    if(speed)
        SHQ_TRY(sc.alloc(&d_speed, (size_t) n));
    SHQ_TRY(sc.mark(s));
    SHQ_HIP(hipMemcpyAsync(d_seeds, seeds.data(), sizeof(uint32_t) * ncol, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * 3 * NK, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_vel, vel, sizeof(float) * 3 * n, hipMemcpyHostToDevice, s));
    SHQ_TRY(sc.mark(s)); /* ev[1]: uploaded */
    const dim3 grid(nblk(ncol, TW));
    thermal_speeds_kernel<<<grid, dim3(TW), 0, s>>>(N, (int) ncol, p->v_amp, d_seeds, d_tab, d_vel, d_dvel, d_speed);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(sc.mark(s)); /* ev[2]: the kernel */
    SHQ_HIP(hipMemcpyAsync(vel, d_vel, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, s));
    if(dvel)
        SHQ_HIP(hipMemcpyAsync(dvel, d_dvel, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
    if(speed)
        SHQ_HIP(hipMemcpyAsync(speed, d_speed, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    SHQ_TRY(sc.mark(s)); /* ev[3]: downloaded */
    SHQ_HIP(hipStreamSynchronize(s));
    ctx->thermal_ms[0] = sc.ms(0, 1);
    ctx->thermal_ms[1] = sc.ms(1, 2);
    ctx->thermal_ms[2] = sc.ms(0, 3);
    return SHQ_OK;
}
