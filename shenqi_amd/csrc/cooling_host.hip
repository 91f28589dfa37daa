/* cooling_host.hip — the host side of the radiative cooling that needs no device: the caller's tables in the engine's layout, and
 * shq_cooling_eval_host, the engine of cooling_math.hpp driven in a plain loop per particle over host threads.  No kernel here: the file
 * also builds into a stand-alone host program (with the sanitizers, for instance) beside a main that defines shq_set_error. */
#include "common.hpp"
#include <string.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>

/* the caller's tables as the engine reads them: scalars, and the two interleaved rate tables */
int shq_cooling_tables_to_engine(const shq_cooling_tables *t, CoolPar *P, std::vector<double> *ion, std::vector<double> *rates)
{
    SHQ_CHECK(t && t->rate_tables, SHQ_ERR_INVALID, "cooling: NULL tables");
    SHQ_CHECK(t->cooling >= 0 && t->cooling <= 2, SHQ_ERR_INVALID, "cooling: CoolingType %d", t->cooling);
    SHQ_CHECK(std::isfinite(t->density_in_phys_cgs) && t->density_in_phys_cgs > 0 && std::isfinite(t->uu_in_cgs) && t->uu_in_cgs > 0 && std::isfinite(t->tt_in_s) &&
                  t->tt_in_s > 0,
              SHQ_ERR_INVALID, "cooling: the units must be finite and > 0");
    memset(P, 0, sizeof(*P));
    P->cooling = t->cooling;
    P->SelfShieldingOn = t->SelfShieldingOn;
    P->HeliumHeatOn = t->HeliumHeatOn;
    P->MinGasTemp = t->MinGasTemp;
    P->CMBTemperature = t->CMBTemperature;
    P->HeliumHeatThresh = t->HeliumHeatThresh;
    P->HeliumHeatAmp = t->HeliumHeatAmp;
    P->HeliumHeatExp = t->HeliumHeatExp;
    P->rho_crit_baryon = t->rho_crit_baryon;
    P->density_in_phys_cgs = t->density_in_phys_cgs;
    P->uu_in_cgs = t->uu_in_cgs;
    P->tt_in_s = t->tt_in_s;
    P->metal_on = t->metal != nullptr;
    if(t->metal)
        for(int d = 0; d < 3; d++) {
            SHQ_CHECK(t->metal_dims[d] >= 2 && t->metal_dims[d] <= 4096 && std::isfinite(t->metal_min[d]) && std::isfinite(t->metal_max[d]) && t->metal_max[d] > t->metal_min[d],
                      SHQ_ERR_INVALID, "cooling: metal table axis %d: %d nodes over [%g, %g]", d, t->metal_dims[d], t->metal_min[d], t->metal_max[d]);
            P->mdims[d] = t->metal_dims[d];
            P->mmin[d] = t->metal_min[d];
            P->mmax[d] = t->metal_max[d];
        }
    /* temp_tab's rows (cooling_rates.cpp:991-1003): 1 GammaH0, 2 GammaHe0, 3 GammaHep, 4 alphaHp, 5 alphaHep, 6 alphaHepp, 7 collisH0,
     * 8 collisHe0, 9 collisHeP, 10 recombHp, 11 recombHeP, 12 recombHePP, 13 freefree1 */
    const int N = SHQ_COOL_NTAB;
    ion->assign((size_t) N * CI_NION, 0.0);
    rates->assign((size_t) N * CC_NCOOL, 0.0);
    for(int i = 0; i < N; i++) {
        for(int c = 0; c < CI_NION; c++)
            (*ion)[(size_t) i * CI_NION + c] = t->rate_tables[(size_t) (1 + c) * N + i];
        for(int c = 0; c < 7; c++)
            (*rates)[(size_t) i * CC_NCOOL + c] = t->rate_tables[(size_t) (7 + c) * N + i];
    }
    for(double v : *ion)
        SHQ_CHECK(std::isfinite(v), SHQ_ERR_INVALID, "cooling: a rate table entry is not finite");
    for(double v : *rates)
        SHQ_CHECK(std::isfinite(v), SHQ_ERR_INVALID, "cooling: a rate table entry is not finite");
    return SHQ_OK;
}

CoolUV shq_cooling_uv(const shq_cooling_uvbg *u) { return CoolUV{u->gJH0, u->gJHep, u->gJHe0, u->epsH0, u->epsHep, u->epsHe0, u->self_shield_dens, u->zreion}; }

extern "C" int shq_cooling_eval_host(const shq_cooling_tables *tables, int what, int64_t n, const double *rho, const double *u, double *ne, const double *Z,
                                     const uint8_t *heiii, const double *dt, const shq_cooling_uvbg *uvbg, double redshift, double min_egy_spec, double lmfp_heat,
                                     double *out, int32_t *status, int32_t *steps, int nthreads)
{
    SHQ_CHECK(tables && uvbg && n >= 0 && (n == 0 || (rho && u && ne && out && status)), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(what >= 0 && what < COOL_WHAT_N, SHQ_ERR_INVALID, "cooling_eval_host: what = %d", what);
    SHQ_CHECK(what != COOL_WHAT_UNEW || n == 0 || dt, SHQ_ERR_INVALID, "cooling_eval_host: UNEW needs dt");
    CoolPar P;
    std::vector<double> ion, rates;
    SHQ_TRY(shq_cooling_tables_to_engine(tables, &P, &ion, &rates));
    const CoolTabs T{ion.data(), rates.data(), tables->metal};
    const CoolUV uv = shq_cooling_uv(uvbg);
    std::atomic<int64_t> next(0);
    const int64_t grain = 64; /* the cost per particle varies by an order of magnitude: hand out small pieces */
    auto work = [&]() {
        for(;;) {
            const int64_t lo = next.fetch_add(grain);
            if(lo >= n)
                return;
            const int64_t hi = std::min(n, lo + grain);
            for(int64_t k = lo; k < hi; k++) {
                CoolIn in;
                CoolState S;
                cool_eval_in(P, what, rho[k], u[k], Z ? Z[k] : 0.0, heiii ? heiii[k] : 0, dt ? dt[k] : 0.0, redshift, min_egy_spec, lmfp_heat, &in);
                cool_init(S, in, ne[k]);
#ifdef SHQ_COOL_NUDGE
                CoolNudge nz; /* the test hook of cooling_math.hpp: never in the library */
#endif
                while(S.phase != COOL_PH_DONE)
                    cool_step(S, P, T, uv, in COOL_NUDGE_PASS);
                status[k] = S.status;
                if(steps)
                    steps[k] = S.steps;
                if(S.status != COOL_ST_OK)
                    continue;
                out[k] = cool_eval_out(P, what, S.out);
                if(cool_eval_updates_ne(what))
                    ne[k] = S.ne_guess;
            }
        }
    };
    unsigned nt = nthreads > 0 ? (unsigned) nthreads : std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > 64 ? 64 : nt);
    if(n < 4 * grain)
        nt = 1;
    std::vector<std::thread> th;
    for(unsigned t = 1; t < nt; t++)
        th.emplace_back(work);
    work();
    for(auto &x : th)
        x.join();
    return SHQ_OK;
}

