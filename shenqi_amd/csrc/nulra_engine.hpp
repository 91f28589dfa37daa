/* nulra_engine.hpp — the state machine of delta_nu_from_power (neutrinos_lra.cpp:136-241) over a backend that owns the arrays: the device
 * (nulra.hip) or the host (nulra_host.hip).  The host owns what decides the branches - ia, nk, scalefact - so a steady-state step on the
 * device waits for nothing.  The stages are the per-index functions below (nulra_math.hpp has their arithmetic): a backend runs each over
 * its index range, one thread or one loop pass per index. */
#ifndef SHQ_NULRA_ENGINE_HPP
#define SHQ_NULRA_ENGINE_HPP

#include "../../include/shenqi_hip.h"
#include "nulra_math.hpp"
#include <math.h>
#include <cmath>

void shq_set_error(const char *fmt, ...);

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

/* the arrays of one state, on the device or on the host */
struct NuArr {
    int nk_alloc, namax, nbins_cap, ntab;
    double *wavenum, *delta_nu_last, *delta_nu_init, *delta_tot, *power_in, *ratio_raw, *logwav, *slope_w, *partial; /* [nk_alloc]; delta_tot x namax, partial x 3 */
    double *kk_nz, *pw_nz, *logk_nz, *logp_nz, *slope_nz, *ratio_nz, *slope_r;                                     /* [nbins_cap] */
    int32_t *nzidx;  /* [nbins_cap] the non-empty bins in order */
    int32_t *status; /* [0] != 0: a NaN in delta_nu_last (endrun 2004); sticky */
    const double *tlogk, *tT, *tslope; /* the IC transfer table and its makima slopes */
};

/* powerspectrum_sum's tail, the square root, and the logs the rebinning and the final spline want; i < nnz */
NUHD void nulra_op_compact(const NuArr &A, const double *sums, int nbins, double BoxMpc, int i)
{
    double kk, d;
    nulra_bin(sums, nbins, A.nzidx[i], BoxMpc, &kk, &d);
    A.kk_nz[i] = kk;
    A.pw_nz[i] = d;
    A.logk_nz[i] = log(kk);
    A.logp_nz[i] = log(d);
}

/* delta_tot_first_init (:117-128); i < nk = nnz */
NUHD void nulra_op_first_init(const NuArr &A, int i, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
{
    const double k = A.kk_nz[i];
    const double T = makima_eval(A.ntab, A.tlogk, A.tT, A.tslope, log10(k));
    A.delta_nu_init[i] = A.pw_nz[i] * T;
    A.delta_tot[(size_t) i * A.namax] = nulra_delta_tot(A.delta_nu_init[i], A.pw_nz[i], OmegaNua3, Omeganonu, OmegaNu1, partnu);
    A.wavenum[i] = k;
}

NUHD void nulra_op_slope_nz(const NuArr &A, int nnz, int i) { A.slope_nz[i] = makima_slope_at(nnz, A.logk_nz, A.logp_nz, i); }

/* Power_in, rebinned in log space when nk differs from the number of non-empty bins (:151-175); i < nk */
NUHD void nulra_op_power_in(const NuArr &A, int i, int rebin, int nnz, int ia)
{
    if(!rebin) {
        A.power_in[i] = A.pw_nz[i];
        return;
    }
    const double logk = log(A.wavenum[i]);
    if(A.logk_nz[nnz - 1] < logk || A.logk_nz[0] > logk)
        A.power_in[i] = A.delta_tot[(size_t) i * A.namax + ia - 1];
    else
        A.power_in[i] = exp(makima_eval(nnz, A.logk_nz, A.logp_nz, A.slope_nz, logk));
}

/* update_delta_tot's loop body (:523-525) */
NUHD void nulra_op_update(const NuArr &A, int i, int col, double OmegaNua3, double Omeganonu, double OmegaNu1, double partnu)
{
    A.delta_tot[(size_t) i * A.namax + col] = nulra_delta_tot(A.delta_nu_last[i], A.power_in[i], OmegaNua3, Omeganonu, OmegaNu1, partnu);
}

/* get_delta_nu_combined's sum over the species (:492-503), in their order */
NUHD void nulra_op_combine(const NuArr &A, int i, int ns, const double *frac)
{
    double v = 0;
    for(int s = 0; s < ns; s++)
        v += A.partial[(size_t) s * A.nk_alloc + i] * frac[s];
    A.delta_nu_last[i] = v;
}

/* the NaN test, the clamp and delta_nu / Power_in (:214-222) */
NUHD void nulra_op_ratio_raw(const NuArr &A, int i)
{
    double v = A.delta_nu_last[i];
    if(v != v)
        A.status[0] = 1; /* every writer stores the same value */
    if(v < 0)
        v = 0;
    A.delta_nu_last[i] = v;
    A.ratio_raw[i] = v / A.power_in[i];
    A.logwav[i] = log(A.wavenum[i]);
}

NUHD void nulra_op_slope_w(const NuArr &A, int nk, int i) { A.slope_w[i] = makima_slope_at(nk, A.logwav, A.ratio_raw, i); }

/* the ratio on the non-empty bins, rebinned back when necessary (:224-239); a log k outside the state's bins takes the end bin's ratio
 * (the reference clamps the upper end and leaves the lower one to a boost exception); i < nnz */
NUHD void nulra_op_ratio_nz(const NuArr &A, int i, int rebin, int nk)
{
    if(!rebin) {
        A.ratio_nz[i] = A.ratio_raw[i];
        return;
    }
    const double lk = A.logk_nz[i];
    if(lk >= A.logwav[nk - 1])
        A.ratio_nz[i] = A.ratio_raw[nk - 1];
    else if(lk <= A.logwav[0])
        A.ratio_nz[i] = A.ratio_raw[0];
    else
        A.ratio_nz[i] = makima_eval(nk, A.logwav, A.ratio_raw, A.slope_w, lk);
}

NUHD void nulra_op_slope_r(const NuArr &A, int nnz, int i) { A.slope_r[i] = makima_slope_at(nnz, A.logk_nz, A.ratio_nz, i); }

/* ---- host only ----------------------------------------------------------------------------------------------------------------- */

#define NU_CHECK(cond, code, ...)                                                                  \
    do {                                                                                           \
        if(!(cond)) {                                                                              \
            shq_set_error(__VA_ARGS__);                                                            \
            return (code);                                                                         \
        }                                                                                          \
    } while(0)
#define NU_TRY(call)                                                                               \
    do {                                                                                           \
        int rc_ = (call);                                                                          \
        if(rc_ != SHQ_OK)                                                                          \
            return rc_;                                                                            \
    } while(0)

/* what the host owns of a state */
struct NuEngine {
    shq_nulra_params p = {};
    std::vector<double> tlogk, tT, tslope; /* copies of the IC transfer table */
    int namax = 0, ia = 0, nk = 0, nnz = 0;
    bool init_done = false, have_step = false;
    std::vector<double> scalefact;
    double nu_prefac = 0;
    double kmax = 0;       /* the largest wavenum of the state */
    double callback_s = 0; /* host time of the last step's node tables (the callbacks are in it) */
    NuNodeTable nodes;

    double partnu_at(double a) const { return p.hybrid_enabled && a > p.nu_crit_time ? p.nufrac_low[0] : 0.0; }
    double nopart(double a) const { return p.omega_nu_nopart(a, 0, p.user); }
    double hubble(double a) const { return p.hubble(a, 0, p.user); }
};

inline int nulra_engine_init(NuEngine &E, const shq_nulra_params *p)
{
    NU_CHECK(p && p->hubble && p->omega_nu_nopart && p->omega_nu_single, SHQ_ERR_INVALID, "nulra_init: null params or callback");
    NU_CHECK(p->nk_allocated >= 4 && p->nk_allocated <= (1 << 20), SHQ_ERR_INVALID, "nulra_init: nk_allocated %d outside [4, 2^20]", p->nk_allocated);
    NU_CHECK(std::isfinite(p->TimeTransfer) && std::isfinite(p->TimeMax) && p->TimeTransfer > 0 && p->TimeMax >= p->TimeTransfer && p->TimeMax < 1e3, SHQ_ERR_INVALID,
             "nulra_init: TimeTransfer %g, TimeMax %g", p->TimeTransfer, p->TimeMax);
    NU_CHECK(p->light > 0 && p->kBtnu > 0 && p->BoxSize_in_MPC > 0 && std::isfinite(p->delta_nu_prefac) && p->Omeganonu > 0, SHQ_ERR_INVALID,
             "nulra_init: light, kBtnu, BoxSize_in_MPC and Omeganonu must be > 0");
    NU_CHECK(p->NPowerTable >= 4 && p->logk && p->T_nu, SHQ_ERR_INVALID, "nulra_init: the IC transfer table needs at least 4 rows");
    for(int i = 1; i < p->NPowerTable; i++)
        NU_CHECK(p->logk[i] > p->logk[i - 1], SHQ_ERR_INVALID, "nulra_init: the transfer table's logk does not increase at row %d", i);
    E = NuEngine();
    E.p = *p;
    E.tlogk.assign(p->logk, p->logk + p->NPowerTable);
    E.tT.assign(p->T_nu, p->T_nu + p->NPowerTable);
    E.tslope.resize(p->NPowerTable);
    makima_slopes(p->NPowerTable, E.tlogk.data(), E.tT.data(), E.tslope.data());
    E.p.logk = E.p.T_nu = nullptr;
    E.namax = (int) ceil((p->TimeMax - p->TimeTransfer) / 0.008) + 4; /* init_neutrinos_lra, :455 */
    E.scalefact.assign((size_t) E.namax, 0.0);
    return SHQ_OK;
}

inline void nulra_fill_info(const NuEngine &E, int kept, shq_nulra_info *info)
{
    *info = shq_nulra_info();
    info->ia = E.ia;
    info->nk = E.nk;
    info->nonzero = E.nnz;
    info->namax = E.namax;
    info->kept = kept;
    info->nnodes = E.nodes.n;
    info->nu_prefac = E.nu_prefac;
    info->callback_s = E.callback_s;
}

/* get_delta_nu_combined (:487-507) at scale factor a over the Na = ia stored spectra: the node table and the species, then the backend */
template <class B> int nulra_delta_nu_combined(NuEngine &E, B &be, double a)
{
    const shq_nulra_params &P = E.p;
    const int Na = E.ia;
    const double partnu = E.partnu_at(a);
    double rate = 0; /* the truncated J of gravitating particle neutrinos wants its phase resolved (nulra_build_nodes) */
    if(partnu > 0 && !(1 - partnu < 1e-3))
        for(int mi = 0; mi < SHQ_NULRA_NUSPECIES; mi++)
            if(P.degeneracy[mi] > 0 && P.mnu[mi] > 0)
                rate = std::max(rate, E.kmax * std::max(P.vcrit_by_light / 2, P.kBtnu / (2 * P.mnu[mi])));
    nulra_build_nodes(log(P.TimeTransfer), log(a), Na, E.scalefact.data(), P.light, [&](double x) { return E.hubble(x); }, E.nodes, rate);
    NU_CHECK(E.nodes.n >= 0, SHQ_ERR_INVALID,
             "nulra: the phase k fs vcrit of the hybrid neutrinos at k = %g needs more than 2^20 quadrature nodes; are k and light in the same length unit?", E.kmax);
    const double deriv_prefac = P.TimeTransfer * (E.hubble(P.TimeTransfer) / P.light) * P.TimeTransfer;
    const double Omega_nu_tot = E.nopart(a);
    NuSpecies S[SHQ_NULRA_NUSPECIES];
    int ns = 0;
    for(int mi = 0; mi < SHQ_NULRA_NUSPECIES; mi++) {
        if(!(P.degeneracy[mi] > 0))
            continue;
        NuSpecies &s = S[ns++];
        s.mnubykT = P.mnu[mi] / P.kBtnu;
        s.qc = 0;
        s.integrate = Na > 1 && s.mnubykT > 0 && E.nodes.n > 0;
        if(partnu > 0) {
            if(1 - partnu < 1e-3)
                s.integrate = 0;
            else
                s.qc = P.vcrit_by_light * s.mnubykT;
        }
        s.frac = P.degeneracy[mi] * P.omega_nu_single(a, mi, P.user) / Omega_nu_tot;
    }
    return be.delta_nu(E.nodes, Na, E.scalefact.data(), deriv_prefac, P.delta_nu_prefac, P.nufrac_low[0], S, ns, E.nk);
}

/* compute_neutrino_power + delta_nu_from_power.  kept (may be null): 1 the step's spectrum was saved, 0 discarded, -1 no update. */
template <class B> int nulra_engine_step(NuEngine &E, B &be, double Time, double TimeIC, const double *sums, int nbins, int *kept)
{
    const shq_nulra_params &P = E.p;
    NU_CHECK(std::isfinite(Time) && Time > 0 && std::isfinite(TimeIC) && TimeIC > 0, SHQ_ERR_INVALID, "nulra_step: Time %g, TimeIC %g", Time, TimeIC);
    int nnz = 0;
    NU_TRY(be.load_bins(sums, nbins, P.BoxSize_in_MPC, &nnz));
    NU_CHECK(nnz >= 4, SHQ_ERR_INVALID, "nulra_step: %d non-empty P(k) bins, the spline wants 4", nnz);
    if(kept)
        *kept = -1;
    if(!E.init_done) {
        if(E.ia == 0) {
            NU_CHECK(nnz <= P.nk_allocated, SHQ_ERR_INVALID, "nulra_step: %d non-empty bins, %d allocated", nnz, P.nk_allocated);
            double klast = 0;
            NU_TRY(be.last_wavenumber(nnz, &klast));
            NU_CHECK(!(log10(klast) > E.tlogk.back()), SHQ_ERR_INVALID, "nulra_step: want k = %g but the maximum of the transfer table is %g", klast,
                     pow(10, E.tlogk.back()));
            E.nk = nnz;
            E.kmax = klast;
            const double OmegaNua3 = E.nopart(P.TimeTransfer) * pow(P.TimeTransfer, 3);
            NU_TRY(be.first_init(nnz, OmegaNua3, P.Omeganonu, P.OmegaNu1, E.partnu_at(TimeIC)));
            E.scalefact[0] = log(TimeIC);
            E.ia = 1;
        }
        NU_TRY(nulra_delta_nu_combined(E, be, exp(E.scalefact[E.ia - 1])));
        E.init_done = true;
    }
    const int rebin = E.nk != nnz;
    NU_TRY(be.power_in(rebin, nnz, E.nk, E.ia));
    const double partnu = E.partnu_at(Time);
    if(1 - partnu > 1e-3 && log(Time) - E.scalefact[E.ia - 1] > SHQ_NULRA_FLOAT_ACC) {
        NU_CHECK(E.ia < E.namax, SHQ_ERR_INVALID, "nulra_step: the history holds %d spectra, TimeMax allowed no more", E.namax);
        const double OmegaNua3 = E.nopart(Time) * pow(Time, 3);
        E.ia++;
        E.scalefact[E.ia - 1] = log(Time);
        NU_TRY(be.update_delta_tot(E.nk, E.ia - 1, OmegaNua3, P.Omeganonu, P.OmegaNu1, partnu));
        NU_TRY(nulra_delta_nu_combined(E, be, Time));
        if(Time > exp(E.scalefact[E.ia - 2]) + 0.009) {
            NU_TRY(be.update_delta_tot(E.nk, E.ia - 1, OmegaNua3, P.Omeganonu, P.OmegaNu1, partnu));
            if(kept)
                *kept = 1;
        } else {
            E.ia--;
            if(kept)
                *kept = 0;
        }
    }
    const double OmegaNu_nop = E.nopart(Time);
    const double omega_hybrid = P.OmegaNu1 * partnu / pow(Time, 3);
    E.nu_prefac = OmegaNu_nop / (P.Omeganonu / pow(Time, 3) + omega_hybrid);
    E.nnz = nnz;
    NU_TRY(be.finish(rebin, nnz, E.nk));
    E.have_step = true;
    return SHQ_OK;
}

#if defined(__clang__) && (defined(__HIPCC__) || defined(__HIP__))
#pragma clang fp contract(fast)
#endif
#endif
