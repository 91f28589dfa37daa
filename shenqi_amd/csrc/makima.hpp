/* makima.hpp — boost::math::interpolators::makima as this library reads it (shenqi_hip.h, "Two readings of boost"): the modified Akima
 * slopes and the cubic Hermite through them, for the host and the device from one text.  thermal.hip makes its slopes with
 * makima_slopes; nulra_math.hpp uses every function here. */
#ifndef SHQ_MAKIMA_HPP
#define SHQ_MAKIMA_HPP

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#else /* a plain host compiler: the test programs */
#ifndef __host__
#define __host__
#define __device__
#endif
#endif
#include <math.h>

/* every operation rounds on its own, on the host and on the device alike; taken back at the end of this file */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define MKHD __host__ __device__ inline

/* the secant m[j] of the n knots, j = -2 .. n: m[0 .. n-2] from the data, two ghost secants on each side (m[-1] = 2 m[0] - m[1], ...) */
MKHD double makima_secant(int n, const double *x, const double *y, int j)
{
    if(j >= 0 && j < n - 1)
        return (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
    if(j < 0) {
        const double m0 = (y[1] - y[0]) / (x[1] - x[0]), m1 = (y[2] - y[1]) / (x[2] - x[1]);
        const double g1 = 2 * m0 - m1;
        return j == -1 ? g1 : 2 * g1 - m0;
    }
    const double a = (y[n - 1] - y[n - 2]) / (x[n - 1] - x[n - 2]), b = (y[n - 2] - y[n - 3]) / (x[n - 2] - x[n - 3]);
    const double g1 = 2 * a - b;
    return j == n - 1 ? g1 : 2 * g1 - a;
}

/* the modified Akima slope at knot i of n >= 3 knots (boost wants 4) */
MKHD double makima_slope_at(int n, const double *x, const double *y, int i)
{
    const double mm2 = makima_secant(n, x, y, i - 2), mm1 = makima_secant(n, x, y, i - 1), m0 = makima_secant(n, x, y, i),
                 mp1 = makima_secant(n, x, y, i + 1);
    const double w1 = fabs(mp1 - m0) + fabs(mp1 + m0) / 2;
    const double w2 = fabs(mm1 - mm2) + fabs(mm1 + mm2) / 2;
    const double w = w1 + w2;
    return w > 0 ? (w1 * mm1 + w2 * m0) / w : 0.0;
}

/* the modified Akima slopes at the n knots (x, y) */
inline void makima_slopes(int n, const double *x, const double *y, double *s)
{
    for(int i = 0; i < n; i++)
        s[i] = makima_slope_at(n, x, y, i);
}

/* the bin of p: the last knot with x[i] <= p, within [0, n - 2] */
MKHD int makima_bin(int n, const double *x, double p)
{
    int lo = 0, hi = n - 1;
    while(hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if(x[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

/* the four weights of (y[i], s[i], y[i+1], s[i+1]) in the Hermite cubic at p of the bin [x0, x1]:
 * F = (1 - t)^2 (y0 (1 + 2 t) + s0 (p - x0)) + t^2 (y1 (3 - 2 t) + dx s1 (t - 1)) */
MKHD void makima_weights(double x0, double x1, double p, double w[4])
{
    const double dx = x1 - x0, d = p - x0, t = d / dx, omt = 1 - t;
    w[0] = (omt * omt) * (1 + 2 * t);
    w[1] = (omt * omt) * d;
    w[2] = (t * t) * (3 - 2 * t);
    w[3] = (t * t) * (dx * (t - 1));
}

/* the interpolant at p, in the order of operations thermal.hip's kernel uses; p outside the knots continues the end cubic */
MKHD double makima_eval(int n, const double *x, const double *y, const double *s, double p)
{
    const int i = makima_bin(n, x, p);
    const double x0 = x[i], x1 = x[i + 1], y0 = y[i], y1 = y[i + 1], s0 = s[i], s1 = s[i + 1];
    const double dx = x1 - x0, d = p - x0, t = d / dx, omt = 1 - t;
    const double a = y0 * (1 + 2 * t) + s0 * d;
    const double b = y1 * (3 - 2 * t) + (dx * s1) * (t - 1);
    return (omt * omt) * a + (t * t) * b;
}

#if defined(__clang__) && (defined(__HIPCC__) || defined(__HIP__))
#pragma clang fp contract(fast)
#endif
#endif
