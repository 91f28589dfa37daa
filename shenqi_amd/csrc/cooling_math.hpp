/* cooling_math.hpp — the per-particle arithmetic of the radiative cooling of the reference (libgadget/cooling_rates.cpp:293-305, 499-683,
 * 1101-1214; cooling.cpp:42-163; cooling_uvfluc.cpp:321-335 with utils/interp.hpp:58-90), compiled for the device (cooling.hip's
 * kernels) and for the host (shq_cooling_eval_host) from this one text.  DESIGN §3.7l.
 *
 * No rate fit is evaluated here: the thirteen rates are read from the caller's table block (init_cooling_rates' temp_tab) by linear
 * interpolation.  Where the reference would leave the block and call the fit (T >~ 9.8e8 K, or T < 1/e K) the particle is DEFERRED.
 *
 * The solve is a state machine whose step is ONE evaluation of ne_internal.  The reference nests three loops: the bracketing and the
 * bisection of DoCooling, inside each of their iterations the Steffensen fixed point of get_equilib_ne, and inside that two
 * evaluations of ne_internal.  CoolState holds where a particle stands in all three; cool_step advances it by one evaluation and, when
 * the fixed point has converged, by the rate sum and the outer loop's decision that follow.  The host drives it in a plain loop; the
 * kernel drives it per lane, so that lanes in different loops share one instruction stream. */
#ifndef SHQ_COOLING_MATH_HPP
#define SHQ_COOLING_MATH_HPP

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#else /* a plain host compiler: the test programs */
#define __host__
#define __device__
#endif
#include <math.h>
#include <stdint.h>

/* the host and the device round every operation of this file on its own: the bit parity of the host engine with the restatement in
 * tests/ rests on it, and the device stays as close to the host as its libm allows.  The setting is taken back at the end of this file. */
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define CHD __host__ __device__ inline

#define SHQ_COOL_NTAB 1000                        /* NRECOMBTAB */
#define SHQ_COOL_LOGTMAX 0x1.4b927f32bffb8p+4     /* RECOMBTMAX = log(1e9) as glibc rounds it; RECOMBTMIN = 0 */
#define SHQ_COOL_LOG1E4 0x1.26bb1bbb55516p+3      /* log(1e4) */
#define SHQ_COOL_LOG10_32E5 0x1.605460931d620p+2  /* log10(3.2e5) */
#define SHQ_COOL_MAXITER 1000
#define SHQ_COOL_ITERCONV 1e-6
#define SHQ_COOL_HELIUM (1 - 0.76)                /* 1 - HYDROGEN_MASSFRAC */
#define SHQ_COOL_PROTONMASS 1.6726e-24
#define SHQ_COOL_BOLTZMANN 1.38066e-16
#define SHQ_COOL_GAMMA_MINUS1 ((5.0 / 3.0) - 1)
#define SHQ_COOL_THOMPSON 6.65245e-25
#define SHQ_COOL_RAD_CONST 7.565e-15
#define SHQ_COOL_ELECTRONMASS 9.10953e-28
#define SHQ_COOL_LIGHTCGS 2.99792458e10

/* Test hook: with SHQ_COOL_NUDGE defined every log / exp / pow / log10 result is moved by one ulp, up and down in turn, to see on the
 * host how far a libm that rounds differently can carry a result.  Never defined in the library. */
#ifdef SHQ_COOL_NUDGE
struct CoolNudge { unsigned k = 0; };
#define COOL_NUDGE_ARG , CoolNudge &nz
#define COOL_NUDGE_PASS , nz
inline double cool_nudged(double x, CoolNudge &nz) { return (nz.k++ & 1) ? nextafter(x, INFINITY) : nextafter(x, -INFINITY); }
#define COOL_LOG(x) cool_nudged(log(x), nz)
#define COOL_LOG10(x) cool_nudged(log10(x), nz)
#define COOL_EXP(x) cool_nudged(exp(x), nz)
#define COOL_POW(x, y) cool_nudged(pow(x, y), nz)
#else
#define COOL_NUDGE_ARG
#define COOL_NUDGE_PASS
#define COOL_LOG(x) log(x)
#define COOL_LOG10(x) log10(x)
#define COOL_EXP(x) exp(x)
#define COOL_POW(x, y) pow(x, y)
#endif

enum { COOL_KWH92 = 0, COOL_ENZO2NYX = 1, COOL_SHERWOOD = 2 };
/* columns of the two interleaved tables: the entries of one temperature index lie side by side */
enum { CI_GammaH0 = 0, CI_GammaHe0, CI_GammaHep, CI_alphaHp, CI_alphaHep, CI_alphaHepp, CI_NION };
enum { CC_collisH0 = 0, CC_collisHe0, CC_collisHeP, CC_recombHp, CC_recombHeP, CC_recombHePP, CC_freefree1, CC_pad, CC_NCOOL };

/* what the engine reads of cooling_params, cooling_units and the metal table's axes */
struct CoolPar {
    int cooling, SelfShieldingOn, HeliumHeatOn, metal_on;
    double MinGasTemp, CMBTemperature, HeliumHeatThresh, HeliumHeatAmp, HeliumHeatExp, rho_crit_baryon;
    double density_in_phys_cgs, uu_in_cgs, tt_in_s;
    int mdims[3];
    int pad_;
    double mmin[3], mmax[3];
};

struct CoolTabs {
    const double *ion;   /* [SHQ_COOL_NTAB][CI_NION] */
    const double *cool;  /* [SHQ_COOL_NTAB][CC_NCOOL] */
    const double *metal; /* [mdims[0]][mdims[1]][mdims[2]] or NULL */
};

struct CoolUV { /* struct UVBG without J_UV */
    double gJH0, gJHep, gJHe0, epsH0, epsHep, epsHe0, self_shield_dens, zreion;
};

/* one particle's inputs in physical cgs units, constant through its solve */
struct CoolIn {
    double rho;      /* protons / cm^3 */
    double u_old;    /* erg / g, already raised to minegy for UNEW */
    double dt;       /* s */
    double Z, minegy, redshift;
    double lmfp;     /* the long-mean-free-path addend, 0 for a HeIII-ionised particle */
    int what;
};

enum { COOL_WHAT_UNEW = 0, COOL_WHAT_TCOOL, COOL_WHAT_NH0, COOL_WHAT_HE0, COOL_WHAT_HEP, COOL_WHAT_HEPP, COOL_WHAT_TEMP, COOL_WHAT_LAMBDANET, COOL_WHAT_N };
enum { COOL_ST_OK = 0, COOL_ST_DEFERRED = 1, COOL_ST_BADINPUT = 2, COOL_ST_NOCONV = 3, COOL_ST_N };
enum { COOL_PH_FIRST = 0, COOL_PH_UP, COOL_PH_DOWN, COOL_PH_BISECT, COOL_PH_SINGLE, COOL_PH_DONE };

struct CoolState {
    double u;                /* the energy the running rate evaluation is for */
    double u_lower, u_upper;
    double ne0, ne1;         /* the fixed point's iterates, per hydrogen atom */
    double ne_guess;         /* carried from one rate evaluation to the next */
    double out;
    int phase, stage;        /* stage: 0 the next evaluation gives ne1, 1 it gives ne2 */
    int fp_iter, bis_iter;
    int status, steps;
};

/* std::lerp for finite arguments */
CHD double cool_lerp(double a, double b, double t)
{
    if((a <= 0 && b >= 0) || (a >= 0 && b <= 0))
        return t * b + (1 - t) * a;
    if(t == 1)
        return b;
    const double x = a + t * (b - a);
    return ((t > 1) == (b > a)) ? (b < x ? x : b) : (b > x ? x : b);
}

/* get_interpolated_recomb's index and weight; logt is finite.  false: off the table */
CHD bool cool_tab_index(double logt, int *index, double *t)
{
    const double dind = (logt - 0) / (SHQ_COOL_LOGTMAX - 0) * SHQ_COOL_NTAB;
    if(!(dind > -1.0 && dind < SHQ_COOL_NTAB - 1)) /* so that the conversion below is defined */
        return false;
    const int i = (int) dind; /* toward zero: -1 < dind < 0 extrapolates from entry 0 */
    if(i < 0 || i >= SHQ_COOL_NTAB - 1)
        return false;
    *index = i;
    *t = dind - i;
    return true;
}

CHD double cool_self_shield_corr(const CoolPar &P, double nh, double logt, double ssdens COOL_NUDGE_ARG)
{
    if(!P.SelfShieldingOn || nh < ssdens * 0.01)
        return 1;
    const double T4 = COOL_EXP(0.17 * (logt - SHQ_COOL_LOG1E4));
    const double nSSh = 1.003 * ssdens * T4;
    return 0.98 * COOL_POW(1 + COOL_POW(nh / nSSh, 1.64), -2.28) + 0.02 * COOL_POW(1 + nh / nSSh, -0.84);
}

CHD double cool_nH0(const double *ion0, const double *ion1, double t, double ne, const CoolUV &uv, double photofac)
{
    const double alphaHp = cool_lerp(ion0[CI_alphaHp], ion1[CI_alphaHp], t);
    const double GammaeH0 = cool_lerp(ion0[CI_GammaH0], ion1[CI_GammaH0], t);
    double photorate = 0;
    if(uv.gJH0 > 0. && ne > 1e-50)
        photorate = uv.gJH0 / ne * photofac;
    return alphaHp / (alphaHp + GammaeH0 + photorate);
}

struct CoolHe { double nHe0, nHep, nHepp; };

CHD CoolHe cool_nHe(const double *ion0, const double *ion1, double t, double nh, double ne, const CoolUV &uv, double photofac)
{
    const double alphaHep = cool_lerp(ion0[CI_alphaHep], ion1[CI_alphaHep], t);
    const double alphaHepp = cool_lerp(ion0[CI_alphaHepp], ion1[CI_alphaHepp], t);
    double GammaHe0 = cool_lerp(ion0[CI_GammaHe0], ion1[CI_GammaHe0], t);
    double GammaHep = cool_lerp(ion0[CI_GammaHep], ion1[CI_GammaHep], t);
    CoolHe He;
    if(uv.gJHe0 > 0. && ne > 1e-50) {
        GammaHe0 += uv.gJHe0 / ne * photofac;
        GammaHep += uv.gJHep / ne * photofac;
    }
    if(GammaHe0 > 1e-50) {
        He.nHep = nh / (1 + alphaHep / GammaHe0 + GammaHep / alphaHepp);
        He.nHe0 = He.nHep * alphaHep / GammaHe0;
        He.nHepp = He.nHep * GammaHep / alphaHepp;
    }
    else {
        He.nHep = 0;
        He.nHe0 = nh;
        He.nHepp = 0;
    }
    return He;
}

CHD double cool_temp_internal(const CoolPar &P, double nebynh, double ienergy)
{
    const double hy_mass = 1 - SHQ_COOL_HELIUM;
    const double muienergy = 4 / (hy_mass * (3 + 4 * nebynh) + 1) * ienergy;
    const double temp = SHQ_COOL_GAMMA_MINUS1 * SHQ_COOL_PROTONMASS / SHQ_COOL_BOLTZMANN * muienergy;
    if(temp < P.MinGasTemp)
        return P.MinGasTemp;
    return temp;
}

/* ne_internal (:611-621).  *status leaves COOL_ST_OK when logt is not finite or off the table; the value returned is then unused */
CHD double cool_ne_internal(const CoolPar &P, const CoolTabs &T, const CoolUV &uv, double nh, double ienergy, double ne, double *logt, int *status COOL_NUDGE_ARG)
{
    const double helium = SHQ_COOL_HELIUM;
    const double yy = helium / 4 / (1 - helium);
    *logt = COOL_LOG(cool_temp_internal(P, ne / nh, ienergy));
    if(!isfinite(*logt)) {
        *status = COOL_ST_BADINPUT;
        return 0;
    }
    int index;
    double t;
    if(!cool_tab_index(*logt, &index, &t)) {
        *status = COOL_ST_DEFERRED;
        return 0;
    }
    const double photofac = cool_self_shield_corr(P, nh, *logt, uv.self_shield_dens COOL_NUDGE_PASS);
    const double *ion0 = T.ion + (size_t) index * CI_NION, *ion1 = ion0 + CI_NION;
    const double nH0 = cool_nH0(ion0, ion1, t, ne, uv, photofac);
    double nHp = 1. - nH0;
    if(nHp < 0)
        nHp = 0;
    const CoolHe He = cool_nHe(ion0, ion1, t, nh, ne, uv, photofac);
    return nh * nHp + yy * He.nHep + 2 * yy * He.nHepp;
}

/* InterpNLinear<3>::eval (utils/interp.hpp:58-90) */
CHD double cool_metal_rate(const CoolPar &P, const double *ydata, double redshift, double temp, double nHcgs COOL_NUDGE_ARG)
{
    if(!P.metal_on)
        return 0;
    const double x[3] = {redshift, COOL_LOG10(nHcgs), COOL_LOG10(temp)};
    int xi[3];
    double f[3];
    long strides[3];
    long N = 1;
    for(int d = 2; d >= 0; d--) {
        strides[d] = N;
        N *= P.mdims[d];
    }
    for(int d = 0; d < 3; d++) {
        const double step = (P.mmax[d] - P.mmin[d]) / (P.mdims[d] - 1);
        const double xd = (x[d] - P.mmin[d]) / step;
        if(x[d] <= P.mmin[d]) {
            xi[d] = 0;
            f[d] = 0;
        }
        else if(x[d] >= P.mmax[d]) {
            xi[d] = P.mdims[d] - 2;
            f[d] = 1;
        }
        else if(xd == xd) {
            xi[d] = (int) floor(xd);
            if(xi[d] > P.mdims[d] - 2) /* xd rounded up to the last node: the same value from inside the table */
                xi[d] = P.mdims[d] - 2;
            f[d] = xd - xi[d];
        }
        else { /* a NaN coordinate: the table's corner and a NaN weight, no conversion of it */
            xi[d] = 0;
            f[d] = xd;
        }
    }
    double ret = 0;
    const long l0 = strides[0] * xi[0] + strides[1] * xi[1] + strides[2] * xi[2];
    for(int i = 0; i < 8; i++) {
        double filter = 1.0;
        long l = l0;
        for(int d = 0; d < 3; d++) {
            const int foffset = (i & (1 << d)) ? 1 : 0;
            filter *= foffset ? f[d] : (1 - f[d]);
            l += foffset * strides[d];
        }
        ret += ydata[l] * filter;
    }
    return ret;
}

CHD double cool_freefree2(const CoolPar &P, double temp COOL_NUDGE_ARG)
{
    /* cool_FreeFree(temp, 2) of the Enzo2Nyx branch (:872-889) */
    const double lt = 2 * COOL_LOG10(temp / 2);
    double gff;
    if(lt <= SHQ_COOL_LOG10_32E5)
        gff = (0.79464 + 0.1243 * lt);
    else
        gff = (2.13164 - 0.1240 * lt);
    return 1.426e-27 * sqrt(temp) * 4.0 * gff;
}

/* what follows the converged fixed point.  In: logt and ne0 of the convergence.  Out by `what`. */
struct CoolRates { double lambdanet, nebynh, temp, nH0; CoolHe He; };

CHD CoolRates cool_rates(const CoolPar &P, const CoolTabs &T, const CoolUV &uv, const CoolIn &in, double ienergy, double ne0, double logt, bool want_lambda COOL_NUDGE_ARG)
{
    const double helium = SHQ_COOL_HELIUM;
    const double density = in.rho;
    const double nh = density * (1 - helium);
    const double ne = ne0 * nh;       /* get_equilib_ne returns ne0 * nh ... */
    const double nebynh = ne / nh;    /* ... and its callers divide again */
    CoolRates R;
    R.nebynh = nebynh;
    R.temp = cool_temp_internal(P, nebynh, ienergy);
    R.lambdanet = 0;
    int index = 0;
    double t = 0;
    cool_tab_index(logt, &index, &t); /* on the table: the evaluation that converged read it */
    const double photofac = cool_self_shield_corr(P, nh, logt, uv.self_shield_dens COOL_NUDGE_PASS);
    const double yy = helium / 4 / (1 - helium);
    const double *ion0 = T.ion + (size_t) index * CI_NION, *ion1 = ion0 + CI_NION;
    const double nH0 = cool_nH0(ion0, ion1, t, ne, uv, photofac);
    R.nH0 = nH0;
    double nHp = 1. - nH0;
    if(nHp < 0)
        nHp = 0;
    CoolHe He = cool_nHe(ion0, ion1, t, nh, ne, uv, photofac);
    R.He = He;
    if(!want_lambda)
        return R;
    He.nHep *= yy / nh;
    He.nHe0 *= yy / nh;
    He.nHepp *= yy / nh;
    const double *c0 = T.cool + (size_t) index * CC_NCOOL, *c1 = c0 + CC_NCOOL;
    const double LambdaCollis = nebynh * (cool_lerp(c0[CC_collisH0], c1[CC_collisH0], t) * nH0 + cool_lerp(c0[CC_collisHe0], c1[CC_collisHe0], t) * He.nHe0 +
                                          cool_lerp(c0[CC_collisHeP], c1[CC_collisHeP], t) * He.nHep);
    const double LambdaRecomb = nebynh * (cool_lerp(c0[CC_recombHp], c1[CC_recombHp], t) * nHp + cool_lerp(c0[CC_recombHeP], c1[CC_recombHeP], t) * He.nHep +
                                          cool_lerp(c0[CC_recombHePP], c1[CC_recombHePP], t) * He.nHepp);
    const double cff = cool_lerp(c0[CC_freefree1], c1[CC_freefree1], t);
    double LambdaFF;
    if(P.cooling == COOL_ENZO2NYX)
        LambdaFF = nebynh * (cff * (nHp + He.nHep) + cool_freefree2(P, R.temp COOL_NUDGE_PASS) * He.nHepp);
    else
        LambdaFF = nebynh * (cff * (nHp + He.nHep) + 4 * cff * He.nHepp);
    /* cool_InverseCompton (:900-905) */
    const double tcmb_red = P.CMBTemperature * (1 + in.redshift);
    const double compton = 4 * SHQ_COOL_THOMPSON * SHQ_COOL_RAD_CONST / (SHQ_COOL_ELECTRONMASS * SHQ_COOL_LIGHTCGS) * COOL_POW(tcmb_red, 4) * SHQ_COOL_BOLTZMANN * (R.temp - tcmb_red);
    const double LambdaCmptn = nebynh * compton / nh;
    const double Lambda = LambdaCollis + LambdaRecomb + LambdaFF + LambdaCmptn;
    double Heat = (nH0 * uv.epsH0 + He.nHe0 * uv.epsHe0 + He.nHep * uv.epsHep) / nh;
    /* cool_he_reion_factor (:914-924) */
    double hefac = 1.;
    if(P.HeliumHeatOn) {
        const double rho = SHQ_COOL_PROTONMASS * density / (1 - helium);
        double overden = rho / (P.rho_crit_baryon * COOL_POW(1 + in.redshift, 3.0));
        if(overden >= P.HeliumHeatThresh)
            overden = P.HeliumHeatThresh;
        hefac = P.HeliumHeatAmp * COOL_POW(overden, P.HeliumHeatExp);
    }
    Heat *= hefac;
    const double MetalCooling = in.Z * cool_metal_rate(P, T.metal, in.redshift, R.temp, nh COOL_NUDGE_PASS);
    const double LambdaNet = Heat - Lambda - MetalCooling;
    R.lambdanet = LambdaNet * ((1 - helium) * (1 - helium)) * density / SHQ_COOL_PROTONMASS;
    return R;
}

/* start a rate evaluation at energy u: get_equilib_ne's entry (:674-683) */
CHD void cool_begin_eval(CoolState &S, double u)
{
    S.u = u;
    S.ne0 = S.ne_guess <= 0 ? 1.0 : S.ne_guess;
    S.stage = 0;
    S.fp_iter = 0;
}

CHD void cool_finish(CoolState &S, int status, double out)
{
    S.status = status;
    S.out = out;
    S.phase = COOL_PH_DONE;
}

/* the bisection's loop head (cooling.cpp:100-108) */
CHD void cool_bisect_head(CoolState &S, const CoolIn &in)
{
    const double u = 0.5 * (S.u_lower + S.u_upper);
    if(S.u_upper <= in.minegy) {
        cool_finish(S, COOL_ST_OK, in.minegy);
        return;
    }
    S.phase = COOL_PH_BISECT;
    cool_begin_eval(S, u);
}

/* in: rho, u_old in cgs (u_old before the MinEgySpec floor), ne the caller's guess */
CHD void cool_init(CoolState &S, CoolIn &in, double ne)
{
    S.ne_guess = ne;
    S.ne1 = 0;
    S.out = 0;
    S.status = COOL_ST_OK;
    S.steps = 0;
    S.bis_iter = 0;
    S.phase = in.what == COOL_WHAT_UNEW ? COOL_PH_FIRST : COOL_PH_SINGLE;
    if(!(in.rho > 0 && in.u_old > 0 && isfinite(in.rho) && isfinite(in.u_old) && isfinite(ne)) || (in.what == COOL_WHAT_UNEW && !isfinite(in.dt))) {
        cool_finish(S, COOL_ST_BADINPUT, 0);
        return;
    }
    if(in.what == COOL_WHAT_UNEW && in.u_old < in.minegy)
        in.u_old = in.minegy;
    S.u_lower = S.u_upper = in.u_old;
    cool_begin_eval(S, in.u_old);
}

/* One evaluation of ne_internal and what it decides.  Call while S.phase != COOL_PH_DONE. */
CHD void cool_step(CoolState &S, const CoolPar &P, const CoolTabs &T, const CoolUV &uv, const CoolIn &in COOL_NUDGE_ARG)
{
    const double nh = in.rho * (1 - SHQ_COOL_HELIUM);
    double logt;
    int st = COOL_ST_OK;
    const double nein = S.stage == 0 ? S.ne0 : S.ne1;
    const double r = cool_ne_internal(P, T, uv, nh, S.u, nein * nh, &logt, &st COOL_NUDGE_PASS) / nh;
    S.steps++;
    if(st != COOL_ST_OK) {
        cool_finish(S, st, 0);
        return;
    }
    if(S.stage == 1) {
        /* Steffensen's update (:651-660) */
        const double ne2 = r;
        const double d = S.ne0 + ne2 - 2.0 * S.ne1;
        double pp = ne2;
        if(d > 1e-15 || d < -1e-15)
            pp = S.ne0 - (S.ne1 - S.ne0) * (S.ne1 - S.ne0) / d;
        S.ne0 = pp;
        if(S.ne0 < 0)
            S.ne0 = 0;
        S.stage = 0;
        S.fp_iter++;
        if(S.fp_iter >= SHQ_COOL_MAXITER || !isfinite(S.ne0))
            cool_finish(S, COOL_ST_NOCONV, 0);
        return;
    }
    S.ne1 = r;
    if(!(fabs(S.ne1 - S.ne0) < SHQ_COOL_ITERCONV)) {
        S.stage = 1;
        return;
    }
    /* converged (:645-649) */
    S.ne0 = S.ne1;
    const bool want_lambda = in.what == COOL_WHAT_UNEW || in.what == COOL_WHAT_TCOOL || in.what == COOL_WHAT_LAMBDANET;
    const CoolRates R = cool_rates(P, T, uv, in, S.u, S.ne0, logt, want_lambda COOL_NUDGE_PASS);
    S.ne_guess = R.nebynh;
    if(S.phase == COOL_PH_SINGLE) {
        const double yy = SHQ_COOL_HELIUM / 4 / (1 - SHQ_COOL_HELIUM);
        double out;
        switch(in.what) {
            case COOL_WHAT_TCOOL: out = R.lambdanet >= 0 ? 0 : in.u_old / (-R.lambdanet); break;
            case COOL_WHAT_NH0: out = R.nH0; break;
            case COOL_WHAT_HE0: out = yy * R.He.nHe0 / nh; break;
            case COOL_WHAT_HEP: out = yy * R.He.nHep / nh; break;
            case COOL_WHAT_HEPP: out = yy * R.He.nHepp / nh; break;
            case COOL_WHAT_TEMP: out = R.temp; break;
            default: out = R.lambdanet + in.lmfp; break;
        }
        cool_finish(S, COOL_ST_OK, out);
        return;
    }
    const double lam = R.lambdanet + in.lmfp; /* get_lambdanet; lmfp is 0 for a HeIII-ionised particle */
    const double f = S.u - in.u_old - lam * in.dt;
    switch(S.phase) {
        case COOL_PH_FIRST:
            if(f < 0) { /* heating */
                S.phase = COOL_PH_UP;
                S.u_lower = S.u_upper;
                S.u_upper *= 1.1;
                cool_begin_eval(S, S.u_upper);
            }
            else {
                S.phase = COOL_PH_DOWN;
                S.u_upper = S.u_lower;
                S.u_lower /= 1.1;
                if(S.u_upper <= in.minegy)
                    cool_bisect_head(S, in);
                else
                    cool_begin_eval(S, S.u_lower);
            }
            return;
        case COOL_PH_UP:
            if(f < 0) {
                S.u_lower = S.u_upper;
                S.u_upper *= 1.1;
                if(++S.bis_iter >= 100 * SHQ_COOL_MAXITER) /* the reference has no cap here; 1.1^n overflows long before, u becomes inf and the particle BADINPUT */
                    cool_finish(S, COOL_ST_NOCONV, 0);
                else
                    cool_begin_eval(S, S.u_upper);
            }
            else {
                S.bis_iter = 0;
                cool_bisect_head(S, in);
            }
            return;
        case COOL_PH_DOWN:
            if(f > 0) {
                S.u_upper = S.u_lower;
                S.u_lower /= 1.1;
                if(S.u_upper <= in.minegy) {
                    S.bis_iter = 0;
                    cool_bisect_head(S, in);
                }
                else if(++S.bis_iter >= 100 * SHQ_COOL_MAXITER)
                    cool_finish(S, COOL_ST_NOCONV, 0);
                else
                    cool_begin_eval(S, S.u_lower);
            }
            else {
                S.bis_iter = 0;
                cool_bisect_head(S, in);
            }
            return;
        default: { /* COOL_PH_BISECT (cooling.cpp:110-128) */
            const double u = S.u;
            if(f > 0)
                S.u_upper = u;
            else
                S.u_lower = u;
            const double du = S.u_upper - S.u_lower;
            S.bis_iter++;
            if(fabs(du / u) > 1.0e-6 && S.bis_iter < SHQ_COOL_MAXITER)
                cool_bisect_head(S, in);
            else if(S.bis_iter >= SHQ_COOL_MAXITER)
                cool_finish(S, COOL_ST_NOCONV, 0);
            else
                cool_finish(S, COOL_ST_OK, u);
            return;
        }
    }
}

/* the unit conversions of DoCooling / GetCoolingTime / GetNeutralFraction around the engine */
CHD void cool_eval_in(const CoolPar &P, int what, double rho, double u, double Z, int heiii, double dt, double redshift, double min_egy_spec, double lmfp, CoolIn *in)
{
    in->rho = rho * (P.density_in_phys_cgs / SHQ_COOL_PROTONMASS);
    in->u_old = u * P.uu_in_cgs;
    in->minegy = min_egy_spec * P.uu_in_cgs;
    in->dt = dt * P.tt_in_s;
    in->Z = Z;
    in->redshift = redshift;
    in->lmfp = heiii ? 0.0 : lmfp;
    in->what = what;
}
CHD double cool_eval_out(const CoolPar &P, int what, double out)
{
    if(what == COOL_WHAT_UNEW)
        return out / P.uu_in_cgs;
    if(what == COOL_WHAT_TCOOL)
        return out / P.tt_in_s;
    return out;
}
CHD bool cool_eval_updates_ne(int what) { return what == COOL_WHAT_UNEW || what == COOL_WHAT_TCOOL || what == COOL_WHAT_TEMP || what == COOL_WHAT_LAMBDANET; }

/* the pragma above holds to the end of the translation unit: hand whatever includes this file hipcc's default back */
#if defined(__clang__) && (defined(__HIPCC__) || defined(__HIP__))
#pragma clang fp contract(fast)
#endif

#endif
