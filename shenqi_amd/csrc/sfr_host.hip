/* sfr_host.hip — the host side of the star-forming branch that needs no device: the argument checks both entries share, and
 * shq_sfr_eval_host, the engine of sfr_math.hpp driven in a plain loop per particle over host threads.  No kernel here: the file also
 * builds into a stand-alone host program (with the sanitizers, for instance) beside cooling_host.hip and a main that defines
 * shq_set_error. */
#include "common.hpp"
#include "sfr_math.hpp"
#include <string.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>

int shq_sfr_check_args(const shq_sfr_params *par, int what, int64_t n, const shq_sfr_arrays *in, const shq_sfr_eval_step *step, const double *out,
                       const uint8_t *flags_out, const uint8_t *decision, const uint8_t *branch, const int32_t *status)
{
    SHQ_CHECK(par && in && step && n >= 0, SHQ_ERR_INVALID, "sfr_eval: null argument");
    SHQ_CHECK(what >= 0 && what < SHQ_SFR_NWHAT, SHQ_ERR_INVALID, "sfr_eval: what = %d", what);
    SHQ_CHECK(par->Generations >= 1, SHQ_ERR_INVALID, "sfr_eval: Generations = %d", par->Generations);
    SHQ_CHECK(par->BHFeedbackUseTcool >= 0 && par->BHFeedbackUseTcool <= 3, SHQ_ERR_INVALID, "sfr_eval: BHFeedbackUseTcool = %d", par->BHFeedbackUseTcool);
    SHQ_CHECK(n < (1ll << 31), SHQ_ERR_INVALID, "sfr_eval: too many particles");
    if(n == 0)
        return SHQ_OK;
    SHQ_CHECK(in->Density && in->Entropy && in->Ne && in->Metallicity && in->Mass && in->dloga && in->timebin && in->flags && in->ID, SHQ_ERR_INVALID,
              "sfr_eval: a NULL input array");
    SHQ_CHECK(out && flags_out && decision && branch && status, SHQ_ERR_INVALID, "sfr_eval: a NULL output array");
    SHQ_CHECK(step->rnd_table && step->rnd_size > 0, SHQ_ERR_INVALID, "sfr_eval: no random table");
    SHQ_CHECK(std::isfinite(step->hubble) && step->hubble > 0 && std::isfinite(step->a3inv) && step->a3inv > 0 && std::isfinite(step->redshift), SHQ_ERR_INVALID,
              "sfr_eval: redshift, a3inv and hubble must be finite, the last two > 0");
    /* "GradRho not allocated but has SFR_CRITERION_MOLECULAR_H2" (sfr_eff.cpp:822-823) */
    SHQ_CHECK(in->GradRho || (par->StarformationCriterion & 3) != 3, SHQ_ERR_INVALID, "sfr_eval: GradRho is NULL but StarformationCriterion has the H2 bits");
    return SHQ_OK;
}

SfrStep shq_sfr_engine_step(const shq_sfr_eval_step *step, int what, const double *rnd)
{
    SfrStep st;
    memset(&st, 0, sizeof(st));
    st.redshift = step->redshift;
    st.a3inv = step->a3inv;
    st.hubble = step->hubble;
    st.global = shq_cooling_uv(&step->GlobalUVBG);
    st.rnd = rnd;
    st.rndsize = (uint64_t) step->rnd_size;
    st.what = what;
    return st;
}

namespace {
struct HostSink {
    double v[SHQ_SFR_NOUT];
    uint8_t f, d, b;
    void put(int row, double x) { v[row] = x; }
    double get(int row) const { return v[row]; }
    void bytes(uint8_t flags, uint8_t decision, uint8_t branch)
    {
        f = flags;
        d = decision;
        b = branch;
    }
};
} // namespace

extern "C" int shq_sfr_eval_host(const shq_cooling_tables *tables, const shq_sfr_params *par, int what, int64_t n, const shq_sfr_arrays *in,
                                 const shq_sfr_eval_step *step, double *out, uint8_t *flags_out, uint8_t *decision, uint8_t *branch, int32_t *status, int32_t *steps,
                                 int nthreads)
{
    SHQ_CHECK(tables, SHQ_ERR_INVALID, "sfr_eval_host: null tables");
    SHQ_TRY(shq_sfr_check_args(par, what, n, in, step, out, flags_out, decision, branch, status));
    CoolPar P;
    std::vector<double> ion, rates;
    SHQ_TRY(shq_cooling_tables_to_engine(tables, &P, &ion, &rates));
    const CoolTabs T{ion.data(), rates.data(), tables->metal};
    const SfrPar sp = *par;
    const SfrStep st = shq_sfr_engine_step(step, what, step->rnd_table);
    const CoolUV local = shq_cooling_uv(&step->LocalUVBG);
    std::atomic<int64_t> next(0);
    const int64_t grain = 64;
    auto work = [&]() {
        for(;;) {
            const int64_t lo = next.fetch_add(grain);
            if(lo >= n)
                return;
            const int64_t hi = std::min(n, lo + grain);
            for(int64_t k = lo; k < hi; k++) {
                SfrPart p;
                p.Density = in->Density[k];
                p.Entropy = in->Entropy[k];
                p.Ne = in->Ne[k];
                p.Metallicity = in->Metallicity[k];
                p.Mass = in->Mass[k];
                p.Hsml = in->Hsml ? in->Hsml[k] : 0.0;
                p.DivVel = in->DivVel ? in->DivVel[k] : 0.0;
                p.CurlVel = in->CurlVel ? in->CurlVel[k] : 0.0;
                p.GradRho = in->GradRho ? in->GradRho[k] : 0.0;
                p.dloga = in->dloga[k];
                p.DelayTime = in->DelayTime ? in->DelayTime[k] : 0.0;
                p.ID = in->ID[k];
                p.timebin = in->timebin[k];
                p.flags = in->flags[k];
                HostSink sink;
                memset(&sink, 0, sizeof(sink));
                SfrState S;
#ifdef SHQ_COOL_NUDGE
                CoolNudge nz; /* the test hook of cooling_math.hpp: never in the library */
#endif
                sfr_begin(S, sp, P, st, p, sink COOL_NUDGE_PASS);
                while(S.stage != SFR_SG_DONE) {
                    if(S.C.phase != COOL_PH_DONE)
                        cool_step(S.C, P, T, sfr_uv(S, st, local), S.in COOL_NUDGE_PASS);
                    if(S.C.phase == COOL_PH_DONE)
                        sfr_advance(S, sp, P, st, p, sink COOL_NUDGE_PASS);
                }
                status[k] = S.status;
                if(steps)
                    steps[k] = S.steps;
                if(S.status != COOL_ST_OK)
                    continue;
                for(int r = 0; r < SHQ_SFR_NOUT; r++)
                    out[(size_t) r * (size_t) n + (size_t) k] = sink.v[r];
                flags_out[k] = sink.f;
                decision[k] = sink.d;
                branch[k] = sink.b;
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
