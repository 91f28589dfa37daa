/* yields_math.hpp — the per-star arithmetic of metal_return_init / metal_return_copy (libgadget/metal_return.cpp:157-462, 539-569),
 * compiled for the device (yields.hip's kernels) and for the host (shq_yields_init evaluates maxmassfrac with it) from this one text.
 *
 * What the reference approximates is evaluated here in closed form:
 *   - every IMF integral runs over [max(masslow, 1), ...], the power-law branch 0.237912 m^-2.3 of the Chabrier IMF, and its weight is
 *     linear in mass between table nodes (bilinear table; the clamp rule weight(intpmass) mass / intpmass is linear too), so an
 *     integral is a sum over mass segments of  (w_j - s m_j) [P13] + s [P03],  P13(m) = m^-1.3 / -1.3,  P03(m) = m^-0.3 / -0.3,
 *     s the slope of the weight.  The weight is written about the segment's own node (not as alpha + beta m about 0) so that its
 *     intercept stays of the table's size; the differences [P] are taken of the antiderivative's two powers directly: their absolute
 *     error is a few ulp of |P|, which is the scale the integral over the whole table has.
 *   - at fixed metallicity the lifetime table decreases strictly with mass on the bracket (checked at shq_yields_init), so the root
 *     the reference brackets to 0.5 % is the inverse of one linear segment. */
#ifndef SHQ_YIELDS_MATH_HPP
#define SHQ_YIELDS_MATH_HPP

#include <hip/hip_runtime.h>
#include <math.h>

#define SHQ_YIELD_NMETALS 9
#define SHQ_YIELD_HUBBLE 3.2407789e-18       /* h / s (physconst.h) */
#define SHQ_YIELD_SEC_PER_MEGAYEAR 3.155e13
#define YHD __host__ __device__ inline

/* one flat array of doubles holds every table; offsets in doubles */
struct YieldDesc {
    int life_nmet, life_nmass, agb_nmet, agb_nmass, snii_nmet, snii_nmass;
    int o_life_met, o_life_mass, o_life;
    /* per family: the metallicity axis, the mass axis, 2 + NMETALS tables [nmass][nmet] (total mass, total metals, species), and P13 / P03 of
     * the mass nodes */
    int o_agb_met, o_agb_mass, o_agb, o_agb_p13, o_agb_p03;
    int o_snii_met, o_snii_mass, o_snii, o_snii_p13, o_snii_p03;
    int o_sn1a; /* sn1a_total_metals, sn1a_yields[NMETALS] */
    int ndoubles;
    double Sn1aN0, HubbleParam, imf_norm, MAXMASS, SNAGBSWITCH;
    double sn1a_scale;  /* Sn1aN0 / totalSN1a (:309-311) */
    double maxmassfrac; /* :425 */
};

struct YieldFam {
    const double *met, *mass, *z, *p13, *p03;
    int nmet, nmass;
};

YHD YieldFam yield_agb(const double *T, const YieldDesc &d)
{
    return YieldFam{T + d.o_agb_met, T + d.o_agb_mass, T + d.o_agb, T + d.o_agb_p13, T + d.o_agb_p03, d.agb_nmet, d.agb_nmass};
}
YHD YieldFam yield_snii(const double *T, const YieldDesc &d)
{
    return YieldFam{T + d.o_snii_met, T + d.o_snii_mass, T + d.o_snii, T + d.o_snii_p13, T + d.o_snii_p03, d.snii_nmet, d.snii_nmass};
}

YHD double yield_p13(double m) { return pow(m, -1.3) / -1.3; }
YHD double yield_p03(double m) { return pow(m, -0.3) / -0.3; }

/* std::upper_bound(a, a + n, x) - a: the number of entries <= x (the axes have at most a few tens of nodes) */
YHD int yield_upper(const double *a, int n, double x)
{
    int k = 0;
    while(k < n && !(x < a[k]))
        k++;
    return k;
}
/* the cell of Bilinear2D::eval (utils/interp.hpp:17-20) */
YHD int yield_cell(const double *a, int n, double x)
{
    int i = yield_upper(a, n, x) - 1;
    i = i > n - 2 ? n - 2 : i;
    return i < 0 ? 0 : i;
}

/* Bilinear2D::eval (utils/interp.hpp:16-27), with its un-clamped extrapolation */
YHD double yield_bilinear(const double *xs, int nx, const double *ys, int ny, const double *zs, double x, double y)
{
    const int i = yield_cell(xs, nx, x), j = yield_cell(ys, ny, y);
    const double tx = (x - xs[i]) / (xs[i + 1] - xs[i]);
    const double ty = (y - ys[j]) / (ys[j + 1] - ys[j]);
    return (1.0 - tx) * (1.0 - ty) * zs[j * nx + i] + tx * (1.0 - ty) * zs[j * nx + i + 1] + (1.0 - tx) * ty * zs[(j + 1) * nx + i] +
           tx * ty * zs[(j + 1) * nx + i + 1];
}

/* massendlife (:190-195) */
YHD double yield_massendlife(const double *T, const YieldDesc &d, double stellarmetal, double mass, double dtfind)
{
    return yield_bilinear(T + d.o_life_met, d.life_nmet, T + d.o_life_mass, d.life_nmass, T + d.o_life, stellarmetal, mass) / 1e6 - dtfind;
}

/* do_rootfinding (:198-207) for a bracket [mass_low, MAXMASS] with life(mass_low) > dtfind > life(MAXMASS): the segment of the (decreasing)
 * lifetime curve at this metallicity that crosses dtfind, inverted */
YHD double yield_life_root(const double *T, const YieldDesc &d, double stellarmetal, double dtfind, double mass_low)
{
    const double *xs = T + d.o_life_met, *ys = T + d.o_life_mass, *zs = T + d.o_life;
    const int nx = d.life_nmet, ny = d.life_nmass;
    const int i = yield_cell(xs, nx, stellarmetal);
    const double tx = (stellarmetal - xs[i]) / (xs[i + 1] - xs[i]);
    int j = yield_cell(ys, ny, mass_low);
    double la = ((1.0 - tx) * zs[j * nx + i] + tx * zs[j * nx + i + 1]) / 1e6;
    double lb = ((1.0 - tx) * zs[(j + 1) * nx + i] + tx * zs[(j + 1) * nx + i + 1]) / 1e6;
    while(lb > dtfind && j < ny - 2) {
        j++;
        la = lb;
        lb = ((1.0 - tx) * zs[(j + 1) * nx + i] + tx * zs[(j + 1) * nx + i + 1]) / 1e6;
    }
    return ys[j] + (la - dtfind) / (la - lb) * (ys[j + 1] - ys[j]);
}

/* find_mass_bin_limits (:215-254) */
YHD void yield_mass_bin_limits(const double *T, const YieldDesc &d, double *masslow, double *masshigh, double dtstart, double dtend, double stellarmetal)
{
    const double *lmet = T + d.o_life_met;
    if(stellarmetal < lmet[0])
        stellarmetal = lmet[0];
    if(stellarmetal > lmet[d.life_nmet - 1])
        stellarmetal = lmet[d.life_nmet - 1];
    const double agb_m0 = T[d.o_agb_mass];
    /* no stars have died yet */
    if(yield_massendlife(T, d, stellarmetal, d.MAXMASS, dtend) >= 0) {
        *masslow = d.MAXMASS;
        *masshigh = d.MAXMASS;
        return;
    }
    /* all stars die before the end of this timestep */
    if(yield_massendlife(T, d, stellarmetal, agb_m0, dtend) <= 0)
        *masslow = T[d.o_life_mass];
    else
        *masslow = yield_life_root(T, d, stellarmetal, dtend, agb_m0);
    if(yield_massendlife(T, d, stellarmetal, d.MAXMASS, dtstart) >= 0)
        *masshigh = d.MAXMASS;
    else if(yield_massendlife(T, d, stellarmetal, *masslow, dtstart) <= 0)
        *masshigh = *masslow;
    else
        *masshigh = yield_life_root(T, d, stellarmetal, dtstart, *masslow);
}

/* The integrals of chabrier_imf_integ (:267-282) over [lo, hi], 1 <= lo < hi, for the NT tables t0 .. t0 + NT - 1 of a family at one (clamped)
 * metallicity: acc[t].  The four powers of the two limits are this call's only transcendentals; the nodes' come with the tables. */
template <int NT> YHD void yield_imf_integrals(const YieldFam &f, int t0, double metallicity, double lo, double hi, double *acc)
{
    const int nx = f.nmet, ny = f.nmass, tsz = nx * ny;
    const int i = yield_cell(f.met, nx, metallicity);
    const double tx = (metallicity - f.met[i]) / (f.met[i + 1] - f.met[i]);
    const double *z = f.z + (long) t0 * tsz + i;
    for(int t = 0; t < NT; t++)
        acc[t] = 0;
    double pa13 = yield_p13(lo), pa03 = yield_p03(lo);
    const double ph13 = yield_p13(hi), ph03 = yield_p03(hi);
    int jn = yield_upper(f.mass, ny, lo); /* the first node above lo */
    for(;;) {
        const bool last = jn >= ny || f.mass[jn] >= hi;
        const double pb13 = last ? ph13 : f.p13[jn], pb03 = last ? ph03 : f.p03[jn];
        const double d13 = pb13 - pa13, d03 = pb03 - pa03;
        if(jn == 0 || jn >= ny) {
            /* outside the table: weight(edge node) mass / edge mass */
            const int je = jn == 0 ? 0 : ny - 1;
            const double inv = 1.0 / f.mass[je];
            for(int t = 0; t < NT; t++) {
                const double w = (1.0 - tx) * z[t * tsz + je * nx] + tx * z[t * tsz + je * nx + 1];
                acc[t] += w * inv * d03;
            }
        }
        else {
            const double mj = f.mass[jn - 1], rdm = 1.0 / (f.mass[jn] - mj);
            for(int t = 0; t < NT; t++) {
                const double wa = (1.0 - tx) * z[t * tsz + (jn - 1) * nx] + tx * z[t * tsz + (jn - 1) * nx + 1];
                const double wb = (1.0 - tx) * z[t * tsz + jn * nx] + tx * z[t * tsz + jn * nx + 1];
                const double s = (wb - wa) * rdm;
                acc[t] += (wa - s * mj) * d13 + s * d03;
            }
        }
        if(last)
            break;
        pa13 = pb13;
        pa03 = pb03;
        jn++;
    }
    for(int t = 0; t < NT; t++)
        acc[t] *= 0.237912;
}

/* compute_agb_yield + compute_snii_yield (:316-366) for NT tables from t0, summed: out[t] */
template <int NT> YHD void yield_agb_snii(const double *T, const YieldDesc &d, int t0, double stellarmetal, double masslow, double masshigh, double *out)
{
    double acc[NT];
    for(int t = 0; t < NT; t++)
        out[t] = 0;
    {
        const YieldFam f = yield_agb(T, d);
        double hi = masshigh > d.SNAGBSWITCH ? d.SNAGBSWITCH : masshigh;
        double lo = masslow < f.mass[0] ? f.mass[0] : masslow;
        double Z = stellarmetal > f.met[f.nmet - 1] ? f.met[f.nmet - 1] : stellarmetal;
        Z = Z < f.met[0] ? f.met[0] : Z;
        if(lo < hi) {
            yield_imf_integrals<NT>(f, t0, Z, lo, hi, acc);
            for(int t = 0; t < NT; t++)
                out[t] += acc[t];
        }
    }
    {
        const YieldFam f = yield_snii(T, d);
        double hi = masshigh > f.mass[f.nmass - 1] ? f.mass[f.nmass - 1] : masshigh;
        double lo = masslow < d.SNAGBSWITCH ? d.SNAGBSWITCH : masslow;
        double Z = stellarmetal > f.met[f.nmet - 1] ? f.met[f.nmet - 1] : stellarmetal;
        Z = Z < f.met[0] ? f.met[0] : Z;
        if(lo < hi) {
            yield_imf_integrals<NT>(f, t0, Z, lo, hi, acc);
            for(int t = 0; t < NT; t++)
                out[t] += acc[t];
        }
    }
}

/* sn1a_number (:298-313) */
YHD double yield_sn1a_number(const YieldDesc &d, double dtmyrstart, double dtmyrend)
{
    const double sn1aindex = 1.12, tau8msun = 40;
    if(dtmyrend < tau8msun)
        return 0;
    if(dtmyrstart < tau8msun)
        dtmyrstart = tau8msun;
    return d.sn1a_scale * (pow(dtmyrstart / tau8msun, 1 - sn1aindex) - pow(dtmyrend / tau8msun, 1 - sn1aindex));
}

/* mass_yield (:369-382) */
YHD double yield_mass_yield(const double *T, const YieldDesc &d, double dtmyrstart, double dtmyrend, double stellarmetal, double masslow, double masshigh)
{
    double y[1];
    yield_agb_snii<1>(T, d, 0, stellarmetal, masslow, masshigh, y);
    return y[0] / d.imf_norm + yield_sn1a_number(d, dtmyrstart, dtmyrend) * T[d.o_sn1a];
}

/* metal_yield (:385-407): out[0] = MetalGenerated, out[1 + i] = MetalYields[i], as fractions of the initial SSP */
YHD void yield_metal_yield(const double *T, const YieldDesc &d, double dtmyrstart, double dtmyrend, double stellarmetal, double masslow, double masshigh,
                           double *out)
{
    yield_agb_snii<1 + SHQ_YIELD_NMETALS>(T, d, 1, stellarmetal, masslow, masshigh, out);
    const double n1a = yield_sn1a_number(d, dtmyrstart, dtmyrend);
    for(int t = 0; t < 1 + SHQ_YIELD_NMETALS; t++)
        out[t] = out[t] / d.imf_norm + n1a * T[d.o_sn1a + t];
}

/* Age from the caller's cosmic-time table (n nodes uniform in ln a from loga0, T and dT/dlna per node), by cubic Hermite: the integral
 * of the interpolant from ln(formation) to ln(atime).  Formed so that a young star's age does not come out of the difference of two
 * times of the age of the universe: the width ln(atime / formation) is log1p of the exact difference, the two ends' positions inside
 * their cells differ by that width, and inside a cell p(ub) - p(ua) is taken in factored form. */
YHD double yield_hermite_piece(const double *tt, const double *dt, long k, double dloga, double ua, double ub)
{
    const double y0 = tt[k], y1 = tt[k + 1], m0 = dt[k] * dloga, m1 = dt[k + 1] * dloga;
    /* p(u) = y0 + c1 u + c2 u^2 + c3 u^3 */
    const double dy = y1 - y0;
    const double c1 = m0, c2 = 3 * dy - 2 * m0 - m1, c3 = m0 + m1 - 2 * dy;
    return (ub - ua) * (c1 + c2 * (ub + ua) + c3 * (ub * ub + ub * ua + ua * ua));
}
YHD double yield_age(const double *tt, const double *dt, long n, double loga0, double dloga, double formation, double atime)
{
    const double x1 = (log(formation) - loga0) / dloga;
    long k1 = (long) floor(x1);
    k1 = k1 < 0 ? 0 : (k1 > n - 2 ? n - 2 : k1);
    const double ua = x1 - (double) k1;
    const double w = log1p((atime - formation) / formation) / dloga;
    const double s = ua + w;
    long m = (long) floor(s);
    if(k1 + m > n - 2)
        m = n - 2 - k1;
    if(m <= 0)
        return yield_hermite_piece(tt, dt, k1, dloga, ua, s);
    const long k2 = k1 + m;
    return yield_hermite_piece(tt, dt, k1, dloga, ua, 1.0) + (tt[k2] - tt[k1 + 1]) + yield_hermite_piece(tt, dt, k2, dloga, 0.0, s - (double) m);
}

#endif
