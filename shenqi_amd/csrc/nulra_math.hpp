/* nulra_math.hpp — the arithmetic of the linear-response massive neutrinos of the reference (libgadget/neutrinos_lra.cpp:69-73, 99-241,
 * 487-727; powerspectrum.cpp:71-87; gravpm.cpp:412-427), compiled for the device (nulra.hip's kernels) and for the host (nulra_host.hip)
 * from this one text.  DESIGN 3.14.
 *
 * Every stage is a function of one index (a k bin, a non-empty P(k) bin, a mode k2): the device runs it one thread per index, the host in
 * a plain loop.  The one reduction, the time integral of get_delta_nu, is written per lane (nulra_lane_sum) and folded by a fixed tree
 * (nulra_fold), so the host, the device and two runs of either add the same terms in the same order.
 *
 * The quadrature.  The reference integrates fs(l) / (a H) specialJ(k fs(l) / mnubykT) delta_tot_k(l) over l = log a with an adaptive
 * 61-point Gauss-Kronrod rule per k.  Here the nodes do not depend on k: the knots of the fs spline (Nfs = 16 Na samples) and of the
 * delta_tot history are merged, every merged interval is split so that log(a) - l shrinks by at most a factor 2 per panel (30 levels
 * into the last interval, where fs -> 0 and the integrand of a large k is a spike at the upper limit), and every panel takes 8
 * Gauss-Legendre points.  Per node the table holds fs, the weight w fs / (a H), the history interval and the four Hermite weights of
 * delta_tot there; a (k, species) pair then costs four multiply-adds and one specialJ per node.  H(a) is the caller's, one call per
 * node; the fs samples are cumulative sums of the same panels' 1 / (a^2 H). */
#ifndef SHQ_NULRA_MATH_HPP
#define SHQ_NULRA_MATH_HPP

#include "makima.hpp"
#include <stdint.h>
#include <vector>
#include <algorithm>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define NUHD __host__ __device__ inline

#define SHQ_NULRA_FLOAT_ACC 1e-6 /* FLOAT_ACC, neutrinos_lra.cpp:32 */
#define SHQ_NULRA_LANES 256      /* lanes of one (k, species) integral: the kernel's workgroup, the host's loop */
#define SHQ_NULRA_LEVELS 30      /* halvings into the last merged interval */
#define SHQ_NULRA_GL 8

/* get_delta_tot (neutrinos_lra.cpp:69-73) */
NUHD double nulra_delta_tot(double delta_nu, double delta_cdm, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
{
    const double fcdm = 1 - OmegaNua3 / (Omeganonu + OmegaNu1);
    return fcdm * (delta_cdm + delta_nu * OmegaNua3 / (Omeganonu + OmegaNu1 * partnu));
}

/* specialJ_fit (:561-572) */
NUHD double nulra_specialJ_fit(double x)
{
    if(x <= 0.)
        return 1.;
    const double x2 = x * x, x4 = x2 * x2, x8 = x4 * x4;
    return (1. + 0.0168 * x2 + 0.0407 * x4) / (1. + 2.1734 * x2 + 1.6787 * exp(4.1811 * log(x)) + 0.1467 * x8);
}

/* Jfrac_high (:575-600): the 19 terms share the arguments of J0 and cos, so both are taken once */
NUHD double nulra_Jfrac_high(double x, double qc, double nufrac_low)
{
    const double bj0 = j0(qc * x), cs = cos(qc * x), x2 = x * x;
    double integ = 0, sign = 1; /* -1 * (-1)^n */
    for(int n = 1; n < 20; n++) {
        const double n2 = (double) n * n;
        const double II = (n2 + n2 * n * qc + n * qc * x2 - x2) * qc * bj0 + (2 * n + n2 * qc + qc * x2) * cs;
        integ += sign * exp(-n * qc) / (n2 + x2) / (n2 + x2) * II;
        sign = -sign;
    }
    return integ / (1.5 * 1.202056903159594 * (1 - nufrac_low));
}

/* specialJ (:603-609) */
NUHD double nulra_specialJ(double x, double qc, double nufrac_low) { return qc > 0 ? nulra_Jfrac_high(x, qc, nufrac_low) : nulra_specialJ_fit(x); }

/* the node table of one call, k-independent; h is [4][n] */
struct NuNodes {
    int n;
    const double *W, *fs, *h;
    const int32_t *iv;
};

/* the history row of one k as the nodes read it: Na >= 4 (y[i], s[i]) interleaved, the makima slopes made here; Na < 4 the values alone
 * (the nodes then carry the weights of the interpolating polynomial, the reference's barycentric rational of order Na - 1), zero filled
 * to four entries.  Entry e of max(2 Na, 4). */
NUHD double nulra_row_entry(int Na, const double *sf, const double *y, int e)
{
    if(Na >= 4)
        return (e & 1) ? makima_slope_at(Na, sf, y, e >> 1) : y[e >> 1];
    return e < Na ? y[e] : 0.0;
}
NUHD int nulra_row_len(int Na) { return Na >= 4 ? 2 * Na : 4; }

/* the share of lane `lane` of SHQ_NULRA_LANES in sum_j W_j specialJ(kfac fs_j) delta_tot(l_j), nodes lane, lane + LANES, ... in order */
NUHD double nulra_lane_sum(const NuNodes &N, const double *row, double kfac, double qc, double nufrac_low, int lane)
{
    double acc = 0;
    for(int j = lane; j < N.n; j += SHQ_NULRA_LANES) {
        const double *r = row + 2 * N.iv[j];
        const double d = ((N.h[j] * r[0] + N.h[N.n + j] * r[1]) + N.h[2 * (size_t) N.n + j] * r[2]) + N.h[3 * (size_t) N.n + j] * r[3];
        acc += (N.W[j] * nulra_specialJ(kfac * N.fs[j], qc, nufrac_low)) * d;
    }
    return acc;
}

/* one level of the fixed tree over the lanes' sums: v[i] += v[i + half] for i < half; the caller runs half = LANES / 2 ... 1 */
NUHD void nulra_fold(double *v, int i, int half) { v[i] += v[i + half]; }

/* what one call of get_delta_nu shares between the bins, per species */
struct NuSpecies {
    double mnubykT; /* mnu / kBtnu */
    double qc;      /* vcrit mnubykT while the particle neutrinos gravitate, else 0 */
    double frac;    /* degeneracy * omega_nu_single(a, mi) / omega_nu_nopart(a) */
    int integrate;  /* Na > 1, mnubykT > 0 and the particles are not everything */
};

/* get_delta_nu for one bin and one species (:646-659, :725) given the integral */
NUHD double nulra_delta_nu_single(double k, double delta_nu_init, double fsl_A0a, double deriv_prefac, double delta_nu_prefac, const NuSpecies &S,
                                  double integral)
{
    const double specJ = nulra_specialJ_fit(k * fsl_A0a / (S.mnubykT > 0 ? S.mnubykT : 1));
    double v = specJ * delta_nu_init * (1. + deriv_prefac * fsl_A0a);
    if(S.integrate)
        v += delta_nu_prefac * integral;
    return v;
}

/* powerspectrum_sum's tail for the non-empty bin b (powerspectrum.cpp:73-80) and compute_neutrino_power's square root (gravpm.cpp:314-316) */
NUHD void nulra_bin(const double *sums, int nbins, int b, double BoxMpc, double *kk, double *delta_cdm)
{
    unsigned long long nm;
    const double *pm = sums + 2 * (size_t) nbins + b;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(pm);
    unsigned char *dst = reinterpret_cast<unsigned char *>(&nm);
    for(int q = 0; q < 8; q++)
        dst[q] = src[q];
    double P = sums[b];
    P /= (double) (int64_t) nm;
    P /= sums[3 * (size_t) nbins];
    double k = sums[nbins + b] / (double) (int64_t) nm;
    k *= 2 * M_PI / BoxMpc;
    P *= pow(BoxMpc, 3.0);
    *kk = k;
    *delta_cdm = sqrt(P);
}

/* nufac - 1 of potential_transfer (gravpm.cpp:412-427) for the integer k2 > 0: nu_prefac * spline(log |k|), a log k outside the knots
 * takes the end knot's value */
NUHD double nulra_mode_factor(int nnz, const double *logk, const double *ratio, const double *slope, double nu_prefac, double BoxMpc, long long k2)
{
    double lk = log(sqrt((double) k2) * 2 * M_PI / BoxMpc);
    if(lk <= logk[0])
        return nu_prefac * ratio[0];
    if(lk >= logk[nnz - 1])
        return nu_prefac * ratio[nnz - 1];
    return nu_prefac * makima_eval(nnz, logk, ratio, slope, lk);
}

/* ---- host only: the node table --------------------------------------------------------------------------------------------------- */

struct NuNodeTable {
    int n = 0;
    double fsl_A0a = 0;              /* fslength(log TimeTransfer, log a) */
    std::vector<double> l, W, fs, h; /* h is [4][n] */
    std::vector<int32_t> iv;
    long long hubble_calls = 0;
};

/* The nodes of get_delta_nu at log a = la over the history knots sf[0 .. Na-1], from l0 = log TimeTransfer.  hub(a) is the caller's
 * hubble_function.  Na < 2 (or la <= l0) leaves no nodes but still gives fsl_A0a.  History knots outside (l0, la) add no break, and a
 * node outside them continues the end cubic (the reference's boost spline would throw there).
 * rate > 0 (hybrid neutrinos gravitating: Jfrac_high oscillates as cos(qc x), x = k fs / mnubykT, and decays only as x^-2, so the tail of a
 * large k is an alternating sum that has to be resolved): the panels are cut further until fs changes by at most 1 / rate over each;
 * the caller passes rate = kmax max(vcrit / 2, 1 / (2 mnubykT)), half a radian of phase per point and a step of x below 1.  More than
 * max_panels panels leaves T.n = -1. */
template <class Hub>
void nulra_build_nodes(double l0, double la, int Na, const double *sf, double light, Hub hub, NuNodeTable &T, double rate = 0, long long max_panels = 1 << 17)
{
    static const double gx[4] = {0.1834346424956498049394761, 0.5255324099163289858177390, 0.7966664774136267395915539, 0.9602898564975362316835609};
    static const double gw[4] = {0.3626837833783619829651504, 0.3137066458778872873379622, 0.2223810344533744705443560, 0.1012285362903762591525314};
    T = NuNodeTable();
    if(!(la > l0))
        return;
    /* the fs samples (:682-693); a call without an integral still needs fslength(l0, la) and takes it over 32 samples */
    const int Nfs = Na >= 2 ? 16 * Na : 32;
    std::vector<double> fsx((size_t) Nfs), fsy((size_t) Nfs, 0.0), fss((size_t) Nfs);
    for(int i = 0; i < Nfs; i++)
        fsx[i] = l0 + i * (la - l0) / (Nfs - 1.);
    fsx[Nfs - 1] = la;
    /* merged breaks, each with the fs sample it is (or -1) */
    std::vector<std::pair<double, int>> br;
    for(int i = 0; i < Nfs; i++)
        br.push_back({fsx[i], i});
    if(Na >= 2)
        for(int j = 0; j < Na; j++)
            if(sf[j] > l0 && sf[j] < la && !std::binary_search(fsx.begin(), fsx.end(), sf[j]))
                br.push_back({sf[j], -1});
    std::sort(br.begin(), br.end());
    /* panels in ascending l: [lo, hi) and the fs bin they lie in */
    std::vector<double> plo, phi;
    std::vector<int> pfs, pbr; /* the fs bin; the index of the break at the panel's lower end, or -1 */
    int fsbin = 0;
    for(size_t b = 0; b + 1 < br.size(); b++) {
        if(br[b].second >= 0)
            fsbin = std::min(br[b].second, Nfs - 2);
        const double p = br[b].first, q = br[b + 1].first;
        const bool last = b + 2 == br.size();
        double d = la - p;
        const double dq = la - q;
        bool first = true;
        for(int lev = 0; last ? lev < SHQ_NULRA_LEVELS : d / 2 > dq; lev++) {
            plo.push_back(first ? p : la - d);
            phi.push_back(la - d / 2);
            pfs.push_back(fsbin);
            pbr.push_back(first ? (int) b : -1);
            first = false;
            d /= 2;
        }
        plo.push_back(first ? p : la - d);
        phi.push_back(q);
        pfs.push_back(fsbin);
        pbr.push_back(first ? (int) b : -1);
    }
    int np = (int) plo.size(), n = np * SHQ_NULRA_GL;
    std::vector<double> gl, aH, g;
    /* the 8 points of every panel: l, the Gauss-Legendre weight, a H and fslength's integrand 1 / (a^2 H) (:543-547) */
    auto lay = [&]() {
        np = (int) plo.size();
        n = np * SHQ_NULRA_GL;
        T.l.resize(n); gl.resize(n); aH.resize(n); g.resize(n);
        for(int p = 0; p < np; p++) {
            const double mid = (plo[p] + phi[p]) / 2, half = (phi[p] - plo[p]) / 2;
            for(int q = 0; q < SHQ_NULRA_GL; q++) {
                const int j = p * SHQ_NULRA_GL + q;
                const int c = q < 4 ? 3 - q : q - 4;
                const double l = q < 4 ? mid - half * gx[c] : mid + half * gx[c];
                const double a = exp(l);
                T.l[j] = l;
                gl[j] = gw[c] * half;
                aH[j] = a * hub(a);
                g[j] = 1. / a / aH[j];
            }
        }
        T.hubble_calls += n;
    };
    lay();
    /* fs samples: the integral from the sample to la, accumulated downwards from la so that the small ones keep their digits */
    double cum = 0;
    for(int p = np - 1; p >= 0; p--) {
        double s = 0;
        for(int q = 0; q < SHQ_NULRA_GL; q++)
            s += gl[p * SHQ_NULRA_GL + q] * g[p * SHQ_NULRA_GL + q];
        cum += s;
        if(pbr[p] >= 0 && br[pbr[p]].second >= 0)
            fsy[br[pbr[p]].second] = light * cum;
    }
    T.fsl_A0a = fsy[0];
    if(Na < 2) {
        T.n = 0;
        return;
    }
    makima_slopes(Nfs, fsx.data(), fsy.data(), fss.data());
    auto fs_at = [&](int fb, double l) {
        const double x0 = fsx[fb], x1 = fsx[fb + 1], y0 = fsy[fb], y1 = fsy[fb + 1], s0 = fss[fb], s1 = fss[fb + 1];
        const double dx = x1 - x0, d = l - x0, t = d / dx, omt = 1 - t;
        const double a = y0 * (1 + 2 * t) + s0 * d;
        const double b = y1 * (3 - 2 * t) + (dx * s1) * (t - 1);
        return (omt * omt) * a + (t * t) * b;
    };
    if(rate > 0) { /* the truncated J oscillates in k fs: no panel may span more than 1 / rate of fs */
        std::vector<double> qlo, qhi;
        std::vector<int> qfs;
        for(int p = 0; p < np; p++) {
            const double span = rate * fabs(fs_at(pfs[p], plo[p]) - fs_at(pfs[p], phi[p]));
            const long long nsub = span > 1 ? (long long) ceil(span) : 1;
            if((long long) qlo.size() + nsub > max_panels) {
                T.n = -1; /* too many: the caller reports it */
                return;
            }
            for(long long u = 0; u < nsub; u++) {
                qlo.push_back(u == 0 ? plo[p] : plo[p] + (phi[p] - plo[p]) * u / nsub);
                qhi.push_back(u + 1 == nsub ? phi[p] : plo[p] + (phi[p] - plo[p]) * (u + 1) / nsub);
                qfs.push_back(pfs[p]);
            }
        }
        plo.swap(qlo); phi.swap(qhi); pfs.swap(qfs);
        lay();
    }
    T.n = n;
    T.W.resize(n); T.fs.resize(n); T.h.assign((size_t) 4 * n, 0.0); T.iv.assign(n, 0);
    for(int p = 0; p < np; p++) {
        /* the history interval of the panel: the last knot at or below its lower end, within [0, Na - 2] */
        int iv = 0;
        if(Na >= 4) {
            iv = makima_bin(Na, sf, plo[p]);
        }
        for(int q = 0; q < SHQ_NULRA_GL; q++) {
            const int j = p * SHQ_NULRA_GL + q;
            const double l = T.l[j];
            T.fs[j] = fs_at(pfs[p], l);
            T.W[j] = gl[j] * T.fs[j] / aH[j];
            double w[4] = {0, 0, 0, 0};
            if(Na >= 4) {
                makima_weights(sf[iv], sf[iv + 1], l, w);
                T.iv[j] = iv;
            } else { /* the polynomial through the Na knots: Lagrange weights */
                for(int i = 0; i < Na; i++) {
                    double L = 1;
                    for(int m = 0; m < Na; m++)
                        if(m != i)
                            L *= (l - sf[m]) / (sf[i] - sf[m]);
                    w[i] = L;
                }
                T.iv[j] = 0;
            }
            for(int c = 0; c < 4; c++)
                T.h[(size_t) c * n + j] = w[c];
        }
    }
}

#if defined(__clang__) && (defined(__HIPCC__) || defined(__HIP__))
#pragma clang fp contract(fast)
#endif
#endif
