/* sfr_math.hpp — the per-particle arithmetic of the star-forming branch of the reference (libgadget/sfr_eff.cpp: sfreff_on_eeqos :502-533,
 * the *_sfreff fractions :536-600, cooling_relaxed :633-668, quicklyastarformation :673-692, starformation :698-767, get_sfr_eeqos
 * :771-809, get_starformation_rate_full :811-830, get_egyeff :833-846, find_star_mass :970-991, the H2 and self-gravity factors
 * :1009-1080), compiled for the device (sfr.hip) and for the host (shq_sfr_eval_host) from this one text.  DESIGN §3.7m.
 *
 * A particle needs between zero and three GetCoolingTime solves (five fixed points for a two-phase fraction).  SfrState wraps the
 * CoolState of the running solve; its step is one cool_step, i.e. one evaluation of ne_internal.  When a solve has finished, sfr_advance
 * uses its value and either starts the next solve or finishes the particle.  The driver is
 *     sfr_begin(...); while(S.stage != SFR_SG_DONE) { if(S.C.phase != COOL_PH_DONE) cool_step(S.C, ..., sfr_uv(S, st, local), S.in);
 *                                                     if(S.C.phase == COOL_PH_DONE) sfr_advance(...); }
 * Results leave through a sink (put / get / bytes) as they are formed, and a later stage reads them back from there.  The order of
 * every floating operation is the reference's; the host engine's bit parity with the restatement in tests/ rests on it. */
#ifndef SHQ_SFR_MATH_HPP
#define SHQ_SFR_MATH_HPP

#include "cooling_math.hpp"
#include "shenqi_hip.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define SHQ_SFR_METAL_YIELD 0.02
#define SHQ_SFR_FLAG_BHHEATED 8u /* bit 3 of the flag byte; Generation is its upper four bits */

typedef shq_sfr_params SfrPar;

/* one particle's inputs, constant through its solves */
struct SfrPart {
    double Density, Entropy, Ne, Metallicity, Mass, Hsml, DivVel, CurlVel, GradRho, dloga, DelayTime;
    uint64_t ID;
    int timebin;
    unsigned flags;
};

struct SfrStep {
    double redshift, a3inv, hubble;
    CoolUV global;
    const double *rnd; /* RandTable::Table */
    uint64_t rndsize;
    int what;
    int pad_;
};

enum { SFR_SG_CLAUSE4 = 0, SFR_SG_EGYEFF, SFR_SG_EEQOS, SFR_SG_RELAX, SFR_SG_FRAC_STD, SFR_SG_FRAC_COLD, SFR_SG_FRAC_HOT, SFR_SG_DONE };

/* What a later stage of a particle reads of an earlier one travels through the sink's rows (put / get: the caller's output column on
 * the host, the staging column in global memory on the device), not through this state: a lane then carries the running solve and a
 * few integers through the solve, and nothing else. */
struct SfrState {
    CoolState C; /* the running solve */
    CoolIn in;
    int stage, status, steps;
    int on_eeqos, use_global, relaxed;
    unsigned branch, flags;
};

CHD const CoolUV &sfr_uv(const SfrState &S, const SfrStep &st, const CoolUV &local) { return S.use_global ? st.global : local; }

CHD double sfr_enttou(double density, double a3inv COOL_NUDGE_ARG) { return COOL_EXP(SHQ_COOL_GAMMA_MINUS1 * COOL_LOG(density * a3inv)) / SHQ_COOL_GAMMA_MINUS1; }

CHD bool sfr_has(int val, int flag) { return (flag & val) == flag; }

/* GetCoolingTime / GetNeutralFraction / GetHeliumIonFraction: start the solve */
CHD void sfr_begin_solve(SfrState &S, const CoolPar &P, int stage, int cwhat, double redshift, double u, double rho, double ne, double Z, int use_global)
{
    S.stage = stage;
    S.use_global = use_global;
    cool_eval_in(P, cwhat, rho, u, Z, 0, 0.0, redshift, 0.0, 0.0, &S.in);
    cool_init(S.C, S.in, ne);
}

CHD void sfr_done(SfrState &S, int status)
{
    S.status = status;
    S.stage = SFR_SG_DONE;
    S.C.phase = COOL_PH_DONE;
}

/* get_egyeff (:833-846) up to its GetCoolingTime */
template <class Sink> CHD void sfr_begin_egyeff(SfrState &S, const SfrPar &sp, const CoolPar &P, int stage, double redshift, double dens, Sink &sink COOL_NUDGE_ARG)
{
    const double tsfr = sqrt(sp.PhysDensThresh / (dens)) * sp.MaxSfrTimescale;
    const double factorEVP = COOL_POW(dens / sp.PhysDensThresh, -0.8) * sp.FactorEVP;
    const double egyhot = sp.EgySpecSN / (1 + factorEVP) + sp.EgySpecCold;
    sink.put(SHQ_SFR_O_TSFR, tsfr); /* until get_sfr_eeqos writes its own */
    sink.put(SHQ_SFR_O_EGYHOT, egyhot);
    sfr_begin_solve(S, P, stage, COOL_WHAT_TCOOL, redshift, egyhot, dens, 0.5, 0.0, 1);
}

/* ... and after it (:843-845) */
template <class Sink> CHD double sfr_end_egyeff(const SfrPar &sp, double tcool, Sink &sink)
{
    const double tsfr = sink.get(SHQ_SFR_O_TSFR), egyhot = sink.get(SHQ_SFR_O_EGYHOT);
    const double y = tsfr / tcool * egyhot / (sp.FactorSN * sp.EgySpecSN - (1 - sp.FactorSN) * sp.EgySpecCold);
    const double x = 1 + 1 / (2 * y) - sqrt(1 / y + 1 / (4 * y * y));
    return egyhot * (1 - x) + sp.EgySpecCold * x;
}

/* get_sfr_factor_due_to_h2 (:1009-1045) */
CHD double sfr_factor_h2(const SfrPar &sp, const SfrPart &p, double Z, double atime COOL_NUDGE_ARG)
{
    const double a2 = atime * atime;
    const double zoverzsun = Z / SHQ_SFR_METAL_YIELD;
    const double gradrho_mag = p.GradRho;
    /* ev_NH_from_GradRho(gradrho_mag, Hsml, Density, 1) */
    double ev_NH = 0;
    if(!(p.Density <= 0)) {
        if(gradrho_mag > 0)
            ev_NH = p.Density * p.Density / gradrho_mag;
        ev_NH += p.Density * p.Hsml;
    }
    double tau_fmol = ev_NH / a2;
    tau_fmol *= (0.1 + zoverzsun);
    if(tau_fmol > 0) {
        tau_fmol *= 434.78 * sp.tau_fmol_unit;
        double y = 0.756 * (1 + 3.1 * COOL_POW(zoverzsun, 0.365));
        y = COOL_LOG(1 + 0.6 * y + 0.01 * y * y) / (0.6 * tau_fmol);
        y = 1 - 0.75 * y / (1 + 0.25 * y);
        if(y < 0)
            y = 0;
        if(y > 1)
            y = 1;
        return y;
    }
    return 1.0;
}

/* get_sfr_factor_due_to_selfgravity (:1047-1080) */
CHD double sfr_factor_selfgravity(const SfrPar &sp, const SfrPart &p, double atime, double a3inv, double hubble)
{
    const double a2 = atime * atime;
    double divv = p.DivVel / a2;
    divv += 3.0 * hubble * a2;
    if(sfr_has(sp.StarformationCriterion, 13))
        if(divv >= 0)
            return 0;
    const double dv2abs = (divv * divv + (p.CurlVel / a2) * (p.CurlVel / a2));
    const double alpha_vir = 0.2387 * dv2abs / (sp.GravInternal * p.Density * a3inv);
    double y = 1.0;
    if((alpha_vir < 1.0) || (p.Density * a3inv > 100. * sp.PhysDensThresh))
        y = 66.7;
    else
        y = 0.1;
    if(sfr_has(sp.StarformationCriterion, 21))
        y *= 1.0 / (1.0 + alpha_vir);
    return y;
}

/* the end of the particle: cooling_relaxed's last line (:664-667), find_star_mass, the draw, the split test and the second metallicity
 * addend (:747-766).  trelax: the relaxation time after the tcool < trelax test */
template <class Sink> CHD void sfr_finish_starform(SfrState &S, const SfrPar &sp, const SfrStep &st, const SfrPart &p, double trelax, Sink &sink COOL_NUDGE_ARG)
{
    const double dtime = p.dloga / st.hubble;
    double Entropy = p.Entropy;
    if(S.relaxed) {
        const double egyeff = sink.get(SHQ_SFR_O_EGYEFF), egycurrent = sink.get(SHQ_SFR_O_EGYCURRENT), densityfac = sink.get(SHQ_SFR_O_DENSITYFAC);
        Entropy = (egyeff + (egycurrent - egyeff) * COOL_EXP(-dtime / trelax)) / densityfac;
    }
    /* find_star_mass (:970-991); the quick Lyman-alpha mode does not come here */
    double mass_of_star = sp.avg_baryon_mass / sp.Generations;
    if(mass_of_star > p.Mass)
        mass_of_star = p.Mass;
    if(p.Mass < 2 * mass_of_star || (int) (p.flags >> 4) > sp.Generations)
        mass_of_star = p.Mass;
    const double prob = sink.get(SHQ_SFR_O_DM) / mass_of_star;
    const double draw = st.rnd[(p.ID + 1) % st.rndsize];
    const int form_star = draw < prob;
    int decision = 0;
    if(form_star)
        decision = (p.Mass >= 1.1 * mass_of_star) ? 2 : 1;
    double Z = sink.get(SHQ_SFR_O_METALLICITY); /* with the first addend */
    if(!form_star || decision == 2) {
        const double w = st.rnd[p.ID % st.rndsize];
        const double frac = sink.get(SHQ_SFR_O_FRAC);
        Z += (1 - w) * SHQ_SFR_METAL_YIELD * frac / sp.Generations;
    }
    if(form_star)
        S.branch |= 16u;
    sink.put(SHQ_SFR_O_METALLICITY, Z);
    sink.put(SHQ_SFR_O_ENTROPY, Entropy);
    sink.put(SHQ_SFR_O_MASS_OF_STAR, mass_of_star);
    sink.put(SHQ_SFR_O_PROB, prob);
    sink.put(SHQ_SFR_O_TRELAX_USED, trelax);
    sink.bytes((uint8_t) S.flags, (uint8_t) decision, (uint8_t) S.branch);
    sfr_done(S, COOL_ST_OK);
}

/* starformation (:698-745) after get_sfr_eeqos, and cooling_relaxed (:633-663) up to its GetCoolingTime.  The six sfr_eeqos_data rows
 * are in the sink. */
template <class Sink>
CHD void sfr_mid_starform(SfrState &S, const SfrPar &sp, const CoolPar &P, const SfrStep &st, const SfrPart &p, Sink &sink COOL_NUDGE_ARG)
{
    const double dtime = p.dloga / st.hubble;
    const double tsfr = sink.get(SHQ_SFR_O_TSFR), cloudfrac = sink.get(SHQ_SFR_O_CLOUDFRAC), ne = sink.get(SHQ_SFR_O_NE_EEQOS);
    sink.put(SHQ_SFR_O_DTIME, dtime);
    const double atime = 1 / (1 + st.redshift);
    /* get_starformation_rate_full (:811-830) */
    double smr = 0;
    if(S.on_eeqos) {
        const double cloudmass = cloudfrac * p.Mass;
        smr = (1 - sp.FactorSN) * cloudmass / tsfr;
        if(sfr_has(sp.StarformationCriterion, 3))
            smr *= sfr_factor_h2(sp, p, p.Metallicity, atime COOL_NUDGE_PASS);
        if(sfr_has(sp.StarformationCriterion, 5))
            smr *= sfr_factor_selfgravity(sp, p, atime, st.a3inv, st.hubble);
    }
    const double sm = smr * dtime;
    const double pr = sm / p.Mass;
    const double dM = p.Mass * (1 - COOL_EXP(-pr));
    double Sfr;
    if(dtime > 0)
        Sfr = dM / dtime * sp.UnitSfr_in_solar_per_year;
    else
        Sfr = smr * sp.UnitSfr_in_solar_per_year;
    const double w = st.rnd[p.ID % st.rndsize];
    const double frac = (1 - COOL_EXP(-pr));
    const double Z = p.Metallicity + w * SHQ_SFR_METAL_YIELD * frac / sp.Generations;
    sink.put(SHQ_SFR_O_SMR, smr);
    sink.put(SHQ_SFR_O_SM, sm);
    sink.put(SHQ_SFR_O_DM, dM);
    sink.put(SHQ_SFR_O_SFR, Sfr);
    sink.put(SHQ_SFR_O_NE, ne);
    sink.put(SHQ_SFR_O_METALLICITY, Z);
    sink.put(SHQ_SFR_O_FRAC, frac);
    S.flags = p.flags;
    S.relaxed = 0;
    const double trelax = sink.get(SHQ_SFR_O_TRELAX);
    if(p.dloga > 0 && p.timebin) {
        /* cooling_relaxed (:633-668) */
        S.relaxed = 1;
        S.branch |= 32u;
        const double egyhot = sink.get(SHQ_SFR_O_EGYHOT);
        const double egyeff = sp.EgySpecCold * cloudfrac + (1 - cloudfrac) * egyhot;
        const double densityfac = sfr_enttou(p.Density, st.a3inv COOL_NUDGE_PASS);
        const double egycurrent = p.Entropy * densityfac;
        sink.put(SHQ_SFR_O_EGYEFF, egyeff);
        sink.put(SHQ_SFR_O_EGYCURRENT, egycurrent);
        sink.put(SHQ_SFR_O_DENSITYFAC, densityfac);
        if(sp.BHFeedbackUseTcool == 3 || (sp.BHFeedbackUseTcool == 1 && ((p.flags & SHQ_SFR_FLAG_BHHEATED) || egycurrent > 5e6))) {
            S.flags = p.flags & ~SHQ_SFR_FLAG_BHHEATED;
            if(egycurrent > egyeff) {
                S.branch |= 4u;
                /* Ne and Metallicity are the values starformation has just written (:736, :741) */
                sfr_begin_solve(S, P, SFR_SG_RELAX, COOL_WHAT_TCOOL, st.redshift, egycurrent, p.Density * st.a3inv, ne, Z, 0);
                return;
            }
        }
    }
    sfr_finish_starform(S, sp, st, p, trelax, sink COOL_NUDGE_PASS);
}

/* get_sfr_eeqos (:771-809) up to its GetCoolingTime; the particle's on_eeqos is known */
template <class Sink>
CHD void sfr_after_flag(SfrState &S, const SfrPar &sp, const CoolPar &P, const SfrStep &st, const SfrPart &p, Sink &sink COOL_NUDGE_ARG)
{
    if(S.on_eeqos)
        S.branch |= 1u;
    if(st.what == SHQ_SFR_ON_EEQOS) {
        sink.bytes((uint8_t) p.flags, 0, (uint8_t) S.branch);
        sfr_done(S, COOL_ST_OK);
        return;
    }
    if(st.what != SHQ_SFR_STARFORM && (sp.QuickLymanAlphaProbability > 0 || !S.on_eeqos)) {
        /* the neutral fraction of standard gas (:550-554, :583-587) */
        const double u = p.Entropy * sfr_enttou(p.Density, st.a3inv COOL_NUDGE_PASS);
        sfr_begin_solve(S, P, SFR_SG_FRAC_STD, COOL_WHAT_NH0 + (st.what - SHQ_SFR_NH0), st.redshift, u, p.Density * st.a3inv, p.Ne, 0.0, 0);
        return;
    }
    /* "Initialise data to something, just in case" (:775-780) */
    sink.put(SHQ_SFR_O_TRELAX, sp.MaxSfrTimescale);
    sink.put(SHQ_SFR_O_TSFR, sp.MaxSfrTimescale);
    sink.put(SHQ_SFR_O_EGYHOT, sp.EgySpecCold);
    sink.put(SHQ_SFR_O_EGYCOLD, sp.EgySpecCold);
    sink.put(SHQ_SFR_O_CLOUDFRAC, 0.0);
    sink.put(SHQ_SFR_O_NE_EEQOS, 0.0);
    if(!S.on_eeqos) { /* "This shall never happen, but just in case" (:782-784) */
        sfr_mid_starform(S, sp, P, st, p, sink COOL_NUDGE_PASS);
        return;
    }
    const double dtime = p.dloga / st.hubble;
    double tsfr = sqrt(sp.PhysDensThresh / (p.Density * st.a3inv)) * sp.MaxSfrTimescale;
    if(sp.BoostSFDenseGas && ((p.Density * st.a3inv) / sp.PhysDensThresh > sp.BoostSFOverDenseFactor))
        tsfr = sp.PhysDensThresh / (p.Density * st.a3inv) * sp.MaxSfrTimescale;
    if(tsfr < dtime && dtime > 0)
        tsfr = dtime;
    const double factorEVP = COOL_POW(p.Density * st.a3inv / sp.PhysDensThresh, -0.8) * sp.FactorEVP;
    const double egyhot = sp.EgySpecSN / (1 + factorEVP) + sp.EgySpecCold;
    sink.put(SHQ_SFR_O_TSFR, tsfr);
    sink.put(SHQ_SFR_O_FACTOREVP, factorEVP);
    sink.put(SHQ_SFR_O_EGYHOT, egyhot);
    sfr_begin_solve(S, P, SFR_SG_EEQOS, COOL_WHAT_TCOOL, st.redshift, egyhot, p.Density * st.a3inv, p.Ne, p.Metallicity, 0);
}

/* quicklyastarformation (:673-692) and what cooling_and_starformation does with a hit (:256-260) */
template <class Sink> CHD void sfr_quicklya(SfrState &S, const SfrPar &sp, const SfrStep &st, const SfrPart &p, Sink &sink COOL_NUDGE_ARG)
{
    int hit = 0;
    if(!(p.Density <= sp.OverDensThresh)) {
        const double unew = p.Entropy * sfr_enttou(p.Density, st.a3inv COOL_NUDGE_PASS);
        const double meanweight = (4 / (8 - 5 * (1 - 0.76)));
        const double temp = unew * meanweight / sp.temp_to_u;
        if(!(temp >= sp.QuickLymanAlphaTempThresh))
            if(st.rnd[(p.ID + 1) % st.rndsize] < sp.QuickLymanAlphaProbability)
                hit = 1;
    }
    sink.put(SHQ_SFR_O_SM, hit ? p.Mass : 0.0);
    sink.put(SHQ_SFR_O_DM, hit ? p.Mass : 0.0); /* sum_sm's addend */
    sink.put(SHQ_SFR_O_NE, p.Ne);
    sink.put(SHQ_SFR_O_METALLICITY, p.Metallicity);
    sink.put(SHQ_SFR_O_ENTROPY, p.Entropy);
    sink.put(SHQ_SFR_O_MASS_OF_STAR, p.Mass);
    sink.bytes((uint8_t) p.flags, (uint8_t) hit, hit ? 16u : 0u);
    sfr_done(S, COOL_ST_OK);
}

template <class Sink>
CHD void sfr_begin(SfrState &S, const SfrPar &sp, const CoolPar &P, const SfrStep &st, const SfrPart &p, Sink &sink COOL_NUDGE_ARG)
{
    S.status = COOL_ST_OK;
    S.steps = 0;
    S.branch = 0;
    S.on_eeqos = 0;
    S.use_global = 1;
    S.relaxed = 0;
    S.flags = p.flags;
    S.C.phase = COOL_PH_DONE;
    S.C.steps = 0;
    S.stage = SFR_SG_DONE;
    if(!(p.Density > 0 && isfinite(p.Density) && isfinite(p.Entropy) && p.Mass > 0 && isfinite(p.Mass) && isfinite(p.dloga))) {
        sfr_done(S, COOL_ST_BADINPUT);
        return;
    }
    if(st.what == SHQ_SFR_EGYEFF) {
        sfr_begin_egyeff(S, sp, P, SFR_SG_EGYEFF, st.redshift, p.Density, sink COOL_NUDGE_PASS);
        return;
    }
    if(st.what == SHQ_SFR_STARFORM && sp.QuickLymanAlphaProbability > 0) {
        sfr_quicklya(S, sp, st, p, sink COOL_NUDGE_PASS);
        return;
    }
    /* sfreff_on_eeqos (:502-533).  Under QuickLymanAlphaProbability > 0 the fractions do not evaluate it: "QuickLymanAlphaProbability > 0 ||
     * !sfreff_on_eeqos(...)" (:550, :583) */
    int flag = 0;
    if(!(st.what >= SHQ_SFR_NH0 && st.what <= SHQ_SFR_HEPP && sp.QuickLymanAlphaProbability > 0)) {
        if(p.Density * st.a3inv >= sp.PhysDensThresh)
            flag = 1;
        if(p.Density < sp.OverDensThresh)
            flag = 0;
        if(p.DelayTime > 0)
            flag = 0;
    }
    S.on_eeqos = flag;
    if(flag == 1 && sp.BHFeedbackUseTcool == 2) {
        /* the reference passes its own redshift and the Density as it stands in the record (:523-525) */
        const double redshift = cbrt(st.a3inv) - 1;
        sfr_begin_egyeff(S, sp, P, SFR_SG_CLAUSE4, redshift, p.Density, sink COOL_NUDGE_PASS);
        return;
    }
    sfr_after_flag(S, sp, P, st, p, sink COOL_NUDGE_PASS);
}

/* the running solve has ended: use its value */
template <class Sink>
CHD void sfr_advance(SfrState &S, const SfrPar &sp, const CoolPar &P, const SfrStep &st, const SfrPart &p, Sink &sink COOL_NUDGE_ARG)
{
    S.steps += S.C.steps;
    S.C.steps = 0;
    if(S.C.status != COOL_ST_OK) {
        sfr_done(S, S.C.status);
        return;
    }
    const double out = cool_eval_out(P, S.in.what, S.C.out);
    switch(S.stage) {
        case SFR_SG_EGYEFF:
            sink.put(SHQ_SFR_O_QUERY, sfr_end_egyeff(sp, out, sink));
            sink.bytes((uint8_t) p.flags, 0, 0);
            sfr_done(S, COOL_ST_OK);
            return;
        case SFR_SG_CLAUSE4: {
            const double egyeff = sfr_end_egyeff(sp, out, sink);
            sink.put(SHQ_SFR_O_TSFR, 0.0); /* get_egyeff's own, no output of this mode */
            sink.put(SHQ_SFR_O_EGYHOT, 0.0);
            const double enttou = sfr_enttou(p.Density, st.a3inv COOL_NUDGE_PASS);
            const double unew = p.Entropy * enttou;
            S.branch |= 2u;
            sink.put(SHQ_SFR_O_EGYEFF4, egyeff);
            if(unew >= egyeff * 3.2)
                S.on_eeqos = 0;
            sfr_after_flag(S, sp, P, st, p, sink COOL_NUDGE_PASS);
            return;
        }
        case SFR_SG_EEQOS: {
            const double tcool = out;
            const double tsfr = sink.get(SHQ_SFR_O_TSFR), egyhot = sink.get(SHQ_SFR_O_EGYHOT), factorEVP = sink.get(SHQ_SFR_O_FACTOREVP);
            const double ne = S.C.ne_guess;
            const double y = tsfr / tcool * egyhot / (sp.FactorSN * sp.EgySpecSN - (1 - sp.FactorSN) * sp.EgySpecCold);
            const double cloudfrac = 1 + 1 / (2 * y) - sqrt(1 / y + 1 / (4 * y * y));
            const double trelax = tsfr * (1 - cloudfrac) / cloudfrac / (sp.FactorSN * (1 + factorEVP));
            sink.put(SHQ_SFR_O_NE_EEQOS, ne);
            sink.put(SHQ_SFR_O_CLOUDFRAC, cloudfrac);
            sink.put(SHQ_SFR_O_TRELAX, trelax);
            if(st.what == SHQ_SFR_STARFORM) {
                sfr_mid_starform(S, sp, P, st, p, sink COOL_NUDGE_PASS);
                return;
            }
            sfr_begin_solve(S, P, SFR_SG_FRAC_COLD, COOL_WHAT_NH0 + (st.what - SHQ_SFR_NH0), st.redshift, sp.EgySpecCold, p.Density * st.a3inv, ne, 0.0, 0);
            return;
        }
        case SFR_SG_RELAX: {
            const double tcool = out;
            double trelax = sink.get(SHQ_SFR_O_TRELAX);
            sink.put(SHQ_SFR_O_TCOOL_RELAX, tcool);
            if(tcool < trelax && tcool > 0) {
                trelax = tcool;
                S.branch |= 8u;
            }
            sfr_finish_starform(S, sp, st, p, trelax, sink COOL_NUDGE_PASS);
            return;
        }
        case SFR_SG_FRAC_COLD:
            sink.put(SHQ_SFR_O_QUERY, out); /* the cold phase's, until the mix replaces it */
            sfr_begin_solve(S, P, SFR_SG_FRAC_HOT, S.in.what, st.redshift, sink.get(SHQ_SFR_O_EGYHOT), p.Density * st.a3inv, sink.get(SHQ_SFR_O_NE_EEQOS), 0.0, 0);
            return;
        case SFR_SG_FRAC_HOT: {
            const double cloudfrac = sink.get(SHQ_SFR_O_CLOUDFRAC);
            sink.put(SHQ_SFR_O_QUERY, sink.get(SHQ_SFR_O_QUERY) * cloudfrac + (1 - cloudfrac) * out);
            sink.bytes((uint8_t) p.flags, 0, (uint8_t) S.branch);
            sfr_done(S, COOL_ST_OK);
            return;
        }
        default: /* SFR_SG_FRAC_STD */
            sink.put(SHQ_SFR_O_QUERY, out);
            sink.bytes((uint8_t) p.flags, 0, (uint8_t) S.branch);
            sfr_done(S, COOL_ST_OK);
            return;
    }
}

#if defined(__clang__) && (defined(__HIPCC__) || defined(__HIP__))
#pragma clang fp contract(fast)
#endif

#endif
