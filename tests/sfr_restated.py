"""Line-by-line restatement of the star-forming branch of the reference (libgadget/sfr_eff.cpp; the line numbers below are that file's) in
plain Python, on top of cooling_restated.Cooling.GetCoolingTime and the fraction queries of cooling_restated.Network.  Every operation
goes through the `math` module (glibc's libm, as the C code) in the reference's order, so a C engine that restates the same arithmetic
must agree bit for bit.

This file is the ONLY pin of the library's star formation to the reference: the reference ships no star-formation test and no recorded
values, so nothing here is checked against numbers the reference produced.  What the tests can hold the library to is this reading of
the source, statement by statement.

Two things are not literal.  (1) The reference divides by a cooling time of zero (net heating: y = inf, cloudfrac = 1, trelax = 0,
exp(-dtime / 0) = 0) and relies on IEEE arithmetic; Python floats would raise, so those two divisions go through numpy float64.
(2) The reference evaluates sfreff_on_eeqos up to three times per particle (:249, :783, :813) with unchanged arguments, each with its
own GetCoolingTime under BHFeedbackUseTcool == 2; it is restated once per particle and remembered, and the evaluation counts are those
of one."""
import math

import numpy as np

import cooling_restated as cr

METAL_YIELD = 0.02          # sfr_eff.h:11
SFR_CRITERION_DENSITY, SFR_CRITERION_MOLECULAR_H2, SFR_CRITERION_SELFGRAVITY = 1, 3, 5       # sfr_eff.h:17-22
SFR_CRITERION_CONVERGENT_FLOW, SFR_CRITERION_CONTINUOUS_CUTOFF = 13, 21
BHHEATED = 8                # partmanager.h:19-23: IsGarbage, Swallowed, HeIIIionized, BHHeated, Generation : 4

sqrt, exp, log, pow_ = math.sqrt, math.exp, math.log, math.pow


def HAS(val, flag):         # types.h:20
    return (flag & val) == flag


def _div(a, b):
    """a / b as IEEE does it, zero denominators included"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def default_params(units, **kw):
    """sfr_params as init_cooling_and_star_formation (:857-898) leaves them for the reference's parameter defaults: CritPhysDensity 0.01,
    CritOverDensity 57.7, TempSupernova 5.73e7, TempClouds 1000, FactorSN 0.1, FactorEVP 1000, MaxSfrTimescale 1.5, Generations 2"""
    UnitDensity_in_cgs, UnitLength_in_cm, UnitMass_in_g, UnitTime_in_s, HubbleParam = 6.76991e-22, 3.08568e+21, 1.989e+43, 3.08568e+16, 0.7
    p = dict(StarformationOn=1, StarformationCriterion=SFR_CRITERION_DENSITY, BHFeedbackUseTcool=1, Generations=2, BoostSFDenseGas=0, winds_subgrid=0,
             FactorSN=0.1, FactorEVP=1000.0, MaxSfrTimescale=1.5, QuickLymanAlphaProbability=0.0, QuickLymanAlphaTempThresh=1e5, BoostSFOverDenseFactor=1000.0,
             GravInternal=cr.GRAVITY / UnitLength_in_cm ** 3 * UnitMass_in_g * UnitTime_in_s ** 2)
    p["temp_to_u"] = (1.0 / cr.GAMMA_MINUS1) * (cr.BOLTZMANN / cr.PROTONMASS) / units.uu_in_cgs                                   # :867
    p["UnitSfr_in_solar_per_year"] = (UnitMass_in_g / 1.989e33) / (UnitTime_in_s / 3.155e7)                                       # :869
    p["tau_fmol_unit"] = UnitDensity_in_cgs * HubbleParam * UnitLength_in_cm                                                      # :886
    rhocrit = 3 * 0.1 * 0.1 / (8 * math.pi * p["GravInternal"])
    p["OverDensThresh"] = 57.7 * 0.0464 * rhocrit                                                                                 # :887-888
    p["PhysDensThresh"] = 0.01 * cr.PROTONMASS / cr.HYDROGEN_MASSFRAC / UnitDensity_in_cgs                                        # :890
    meanweight = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)                                                                             # :893
    p["EgySpecCold"] = (p["temp_to_u"] / meanweight) * 1000.0                                                                     # :894
    meanweight = 4 / (8 - 5 * (1 - cr.HYDROGEN_MASSFRAC))                                                                         # :897
    p["EgySpecSN"] = p["temp_to_u"] / meanweight * 5.73e7                                                                         # :898
    p["avg_baryon_mass"] = 1.0
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


class Sfr:
    """the functions of sfr_eff.cpp over one parameter set, one step (redshift, a3inv, hubble, the two UVBGs) and one random table.  A
    particle is a dict with Density, Entropy, Ne, Metallicity, Sfr, DelayTime (SPHP) and Mass, Hsml, ID, TimeBinHydro, flags, dloga, DivVel,
    CurlVel, GradRho; starformation() changes it as the reference changes Part[i] and SPHP(i)."""

    def __init__(self, cool, par, redshift, a3inv, hubble, GlobalUVBG, LocalUVBG, rnd):
        self.cool, self.p = cool, par
        self.redshift, self.a3inv, self.hubble = redshift, a3inv, hubble
        self.GlobalUVBG, self.LocalUVBG = GlobalUVBG, LocalUVBG
        self.rnd = [float(x) for x in rnd]

    def get_random_number(self, id_):                   # utils/system.cpp:56-62
        return self.rnd[id_ % len(self.rnd)]

    # :833-846
    def get_egyeff(self, redshift, dens, uvbg):
        sp = self.p
        tsfr = sqrt(sp["PhysDensThresh"] / (dens)) * sp["MaxSfrTimescale"]                                                          # :836
        factorEVP = pow_(dens / sp["PhysDensThresh"], -0.8) * sp["FactorEVP"]                                                      # :837
        egyhot = sp["EgySpecSN"] / (1 + factorEVP) + sp["EgySpecCold"]                                                             # :838
        self.last_egyeff = dict(tsfr=tsfr, egyhot=egyhot)
        ne = 0.5                                                                                                                    # :840
        tcool, ne = self.cool.GetCoolingTime(redshift, egyhot, dens, uvbg, ne, 0.0)                                                 # :841
        y = _div(tsfr, tcool) * egyhot / (sp["FactorSN"] * sp["EgySpecSN"] - (1 - sp["FactorSN"]) * sp["EgySpecCold"])            # :843
        x = 1 + 1 / (2 * y) - sqrt(1 / y + 1 / (4 * y * y))                                                                         # :844
        return egyhot * (1 - x) + sp["EgySpecCold"] * x                                                                             # :845

    # :502-533
    def sfreff_on_eeqos(self, part, a3inv):
        if "_on_eeqos" in part:
            return part["_on_eeqos"]
        sp = self.p
        flag = 0
        if not sp["StarformationOn"]:                                                                                               # :506
            return 0
        if part["Density"] * a3inv >= sp["PhysDensThresh"]:                                                                         # :510
            flag = 1
        if part["Density"] < sp["OverDensThresh"]:                                                                                  # :513
            flag = 0
        if part["DelayTime"] > 0:                                                                                                   # :516
            flag = 0
        part["_egyeff4"] = 0.0
        if flag == 1 and sp["BHFeedbackUseTcool"] == 2:                                                                             # :521
            redshift = float(np.cbrt(a3inv)) - 1                                                                                    # :523
            uvbg = self.GlobalUVBG                                                                                                  # :524 (the caller's get_global_UVBG)
            egyeff = self.get_egyeff(redshift, part["Density"], uvbg)                                                               # :525
            enttou = cr.entropy_to_u(part["Density"], a3inv)                                                                        # :526
            unew = part["Entropy"] * enttou                                                                                         # :527
            if unew >= egyeff * 3.2:                                                                                                # :529
                flag = 0
            part["_egyeff4"] = egyeff
            part["_clause4"] = True
        part["_on_eeqos"] = flag
        return flag

    # :771-809
    def get_sfr_eeqos(self, part, dtime, local_uvbg, redshift, a3inv):
        sp = self.p
        data = dict(trelax=sp["MaxSfrTimescale"], tsfr=sp["MaxSfrTimescale"], egyhot=sp["EgySpecCold"], egycold=sp["EgySpecCold"], cloudfrac=0, ne=0)   # :775-780
        if not self.sfreff_on_eeqos(part, a3inv):                                                                                   # :783
            return data
        data["ne"] = part["Ne"]                                                                                                     # :786
        data["tsfr"] = sqrt(sp["PhysDensThresh"] / (part["Density"] * a3inv)) * sp["MaxSfrTimescale"]                               # :787
        if sp["BoostSFDenseGas"] and ((part["Density"] * a3inv) / sp["PhysDensThresh"] > sp["BoostSFOverDenseFactor"]):             # :788
            data["tsfr"] = sp["PhysDensThresh"] / (part["Density"] * a3inv) * sp["MaxSfrTimescale"]                                 # :789
        if data["tsfr"] < dtime and dtime > 0:                                                                                      # :794
            data["tsfr"] = dtime
        factorEVP = pow_(part["Density"] * a3inv / sp["PhysDensThresh"], -0.8) * sp["FactorEVP"]                                   # :797
        data["egyhot"] = sp["EgySpecSN"] / (1 + factorEVP) + sp["EgySpecCold"]                                                      # :799
        data["egycold"] = sp["EgySpecCold"]                                                                                         # :800
        tcool, data["ne"] = self.cool.GetCoolingTime(redshift, data["egyhot"], part["Density"] * a3inv, local_uvbg, data["ne"], part["Metallicity"])   # :802
        y = _div(data["tsfr"], tcool) * data["egyhot"] / (sp["FactorSN"] * sp["EgySpecSN"] - (1 - sp["FactorSN"]) * sp["EgySpecCold"])   # :803
        data["cloudfrac"] = 1 + 1 / (2 * y) - sqrt(1 / y + 1 / (4 * y * y))                                                         # :805
        data["trelax"] = data["tsfr"] * (1 - data["cloudfrac"]) / data["cloudfrac"] / (sp["FactorSN"] * (1 + factorEVP))            # :807
        part["_factorEVP"] = factorEVP
        return data

    # :1009-1021
    @staticmethod
    def ev_NH_from_GradRho(gradrho_mag, hsml, rho, include_h):
        if rho <= 0:
            return 0
        ev_NH = 0
        if gradrho_mag > 0:
            ev_NH = rho * rho / gradrho_mag
        if include_h > 0:
            ev_NH += rho * hsml
        return ev_NH

    # :1023-1045
    def get_sfr_factor_due_to_h2(self, part, atime):
        a2 = atime * atime
        zoverzsun = part["Metallicity"] / METAL_YIELD                                                                               # :1029
        gradrho_mag = part["GradRho"]                                                                                               # :1030
        tau_fmol = self.ev_NH_from_GradRho(gradrho_mag, part["Hsml"], part["Density"], 1) / a2                                     # :1032
        tau_fmol *= (0.1 + zoverzsun)                                                                                               # :1033
        if tau_fmol > 0:
            tau_fmol *= 434.78 * self.p["tau_fmol_unit"]                                                                            # :1035
            y = 0.756 * (1 + 3.1 * pow_(zoverzsun, 0.365))                                                                          # :1036
            y = log(1 + 0.6 * y + 0.01 * y * y) / (0.6 * tau_fmol)                                                                  # :1037
            y = 1 - 0.75 * y / (1 + 0.25 * y)                                                                                       # :1038
            if y < 0:
                y = 0
            if y > 1:
                y = 1
            return y
        return 1.0

    # :1047-1080
    def get_sfr_factor_due_to_selfgravity(self, part, atime, a3inv, hubble, GravInternal):
        sp = self.p
        a2 = atime * atime
        divv = part["DivVel"] / a2                                                                                                  # :1049
        divv += 3.0 * hubble * a2                                                                                                   # :1051
        if HAS(sp["StarformationCriterion"], SFR_CRITERION_CONVERGENT_FLOW):
            if divv >= 0:
                return 0                                                                                                            # :1054
        dv2abs = (divv * divv + (part["CurlVel"] / a2) * (part["CurlVel"] / a2))                                                    # :1057-1060
        alpha_vir = 0.2387 * dv2abs / (GravInternal * part["Density"] * a3inv)                                                      # :1061
        y = 1.0
        if (alpha_vir < 1.0) or (part["Density"] * a3inv > 100. * sp["PhysDensThresh"]):                                            # :1065-1066
            y = 66.7
        else:
            y = 0.1
        if HAS(sp["StarformationCriterion"], SFR_CRITERION_CONTINUOUS_CUTOFF):
            y *= 1.0 / (1.0 + alpha_vir)                                                                                            # :1077
        return y

    # :811-830
    def get_starformation_rate_full(self, part, sfr_data, atime, a3inv, hubble, GravInternal):
        sp = self.p
        if not self.sfreff_on_eeqos(part, a3inv):                                                                                   # :813
            return 0
        cloudmass = sfr_data["cloudfrac"] * part["Mass"]                                                                            # :817
        rateOfSF = (1 - sp["FactorSN"]) * cloudmass / sfr_data["tsfr"]                                                              # :819
        if HAS(sp["StarformationCriterion"], SFR_CRITERION_MOLECULAR_H2):
            if part["GradRho"] is None:
                raise RuntimeError("GradRho not allocated but has SFR_CRITERION_MOLECULAR_H2")                                      # :823
            rateOfSF *= self.get_sfr_factor_due_to_h2(part, atime)                                                                  # :824
        if HAS(sp["StarformationCriterion"], SFR_CRITERION_SELFGRAVITY):
            rateOfSF *= self.get_sfr_factor_due_to_selfgravity(part, atime, a3inv, hubble, GravInternal)                            # :827
        return rateOfSF

    # :633-668
    def cooling_relaxed(self, part, dtime, local_uvbg, redshift, a3inv, sfr_data, info):
        sp = self.p
        egyeff = sp["EgySpecCold"] * sfr_data["cloudfrac"] + (1 - sfr_data["cloudfrac"]) * sfr_data["egyhot"]                       # :636
        densityfac = cr.entropy_to_u(part["Density"], a3inv)                                                                        # :637
        egycurrent = part["Entropy"] * densityfac                                                                                   # :638
        trelax = sfr_data["trelax"]                                                                                                 # :639
        info.update(egyeff=egyeff, egycurrent=egycurrent, densityfac=densityfac, relaxed=True)
        if sp["BHFeedbackUseTcool"] == 3 or (sp["BHFeedbackUseTcool"] == 1 and ((part["flags"] & BHHEATED) or egycurrent > 5e6)):  # :646
            if egycurrent > egyeff:                                                                                                 # :648
                ne = part["Ne"]                                                                                                     # :650
                tcool, ne = self.cool.GetCoolingTime(redshift, egycurrent, part["Density"] * a3inv, local_uvbg, ne, part["Metallicity"])   # :652
                info.update(tcool_relax=tcool, tcool_ran=True)
                if tcool < trelax and tcool > 0:                                                                                    # :661
                    trelax = tcool
                    info["tcool_won"] = True
            part["flags"] &= ~BHHEATED                                                                                              # :664
        info["trelax_used"] = trelax
        part["Entropy"] = (egyeff + (egycurrent - egyeff) * exp(_div(-dtime, trelax))) / densityfac                                 # :667

    # :673-692
    def quicklyastarformation(self, part, a3inv):
        sp = self.p
        if part["Density"] <= sp["OverDensThresh"]:                                                                                 # :676
            return 0
        enttou = cr.entropy_to_u(part["Density"], a3inv)
        unew = part["Entropy"] * enttou                                                                                             # :680
        meanweight = (4 / (8 - 5 * (1 - cr.HYDROGEN_MASSFRAC)))                                                                     # :682
        temp = unew * meanweight / sp["temp_to_u"]                                                                                  # :683
        if temp >= sp["QuickLymanAlphaTempThresh"]:                                                                                 # :685
            return 0
        if self.get_random_number(part["ID"] + 1) < sp["QuickLymanAlphaProbability"]:                                               # :688
            return 1
        return 0

    # :970-991
    def find_star_mass(self, part, avg_baryon_mass):
        sp = self.p
        if sp["QuickLymanAlphaProbability"] > 0:
            return part["Mass"]
        mass_of_star = avg_baryon_mass / sp["Generations"]                                                                          # :977
        if mass_of_star > part["Mass"]:
            mass_of_star = part["Mass"]                                                                                             # :980
        if part["Mass"] < 2 * mass_of_star or (part["flags"] >> 4) > sp["Generations"]:                                             # :987
            mass_of_star = part["Mass"]
        return mass_of_star

    # :698-767.  Returns the library's outputs for the particle; part is changed as Part[i] / SPHP(i) are.
    def starformation(self, part):
        sp = self.p
        redshift, a3inv, hubble = self.redshift, self.a3inv, self.hubble
        info = dict(egyeff=0.0, egycurrent=0.0, tcool_relax=0.0, relaxed=False, tcool_ran=False, tcool_won=False, trelax_used=0.0)
        dloga = part["dloga"]                                                                                                       # :702
        dtime = dloga / hubble                                                                                                      # :703
        uvbg = self.LocalUVBG                                                                                                       # :712
        sfr_data = self.get_sfr_eeqos(part, dtime, uvbg, redshift, a3inv)                                                           # :714
        atime = 1 / (1 + redshift)                                                                                                  # :716
        smr = self.get_starformation_rate_full(part, sfr_data, atime, a3inv, hubble, sp["GravInternal"])                            # :717
        sm = smr * dtime                                                                                                            # :719
        p = sm / part["Mass"]                                                                                                       # :722
        dM = part["Mass"] * (1 - exp(-p))                                                                                           # :724
        if dtime > 0:
            part["Sfr"] = dM / dtime * sp["UnitSfr_in_solar_per_year"]                                                              # :729
        else:
            part["Sfr"] = smr * sp["UnitSfr_in_solar_per_year"]                                                                     # :733
        part["Ne"] = sfr_data["ne"]                                                                                                 # :736
        w = self.get_random_number(part["ID"])                                                                                      # :739
        frac = (1 - exp(-p))                                                                                                        # :740
        part["Metallicity"] += w * METAL_YIELD * frac / sp["Generations"]                                                           # :741
        if dloga > 0 and part["TimeBinHydro"]:                                                                                      # :744
            self.cooling_relaxed(part, dtime, uvbg, redshift, a3inv, sfr_data, info)                                                # :745
        else:
            info["trelax_used"] = sfr_data["trelax"]
        mass_of_star = self.find_star_mass(part, sp["avg_baryon_mass"])                                                             # :747
        prob = dM / mass_of_star                                                                                                    # :748
        draw = self.get_random_number(part["ID"] + 1)
        form_star = draw < prob                                                                                                     # :750
        decision = 0
        if form_star:
            decision = 2 if part["Mass"] >= 1.1 * mass_of_star else 1                                                               # :756: slots_split_particle
        if not form_star or decision == 2:                                                                                          # :763
            part["Metallicity"] += (1 - w) * METAL_YIELD * frac / sp["Generations"]                                                 # :764
        return dict(trelax=sfr_data["trelax"], tsfr=sfr_data["tsfr"], egyhot=sfr_data["egyhot"], egycold=sfr_data["egycold"], cloudfrac=sfr_data["cloudfrac"],
                    ne_eeqos=sfr_data["ne"], smr=smr, sm=sm, dM=dM, Sfr=part["Sfr"], Ne=part["Ne"], Metallicity=part["Metallicity"], Entropy=part["Entropy"],
                    mass_of_star=mass_of_star, prob=prob, query=0.0, egyeff4=part.get("_egyeff4", 0.0), tcool_relax=info["tcool_relax"], egyeff=info["egyeff"],
                    egycurrent=info["egycurrent"], trelax_used=info["trelax_used"], dtime=dtime, factorEVP=part.get("_factorEVP", 0.0), densityfac=info.get("densityfac", 0.0), frac=frac, flags=part["flags"], decision=decision, draw=draw,
                    branch=(1 if part["_on_eeqos"] else 0) | (2 if part.get("_clause4") else 0) | (4 if info["tcool_ran"] else 0) | (8 if info["tcool_won"] else 0) |
                    (16 if form_star else 0) | (32 if info["relaxed"] else 0))

    # cooling_and_starformation's quick Lyman-alpha branch (:246-260)
    def quicklya(self, part):
        hit = self.quicklyastarformation(part, self.a3inv)
        sm = part["Mass"] if hit else 0.0
        return dict(sm=sm, dM=sm, Ne=part["Ne"], Metallicity=part["Metallicity"], Entropy=part["Entropy"], mass_of_star=self.find_star_mass(part, 0.0),
                    flags=part["flags"], decision=hit, branch=16 if hit else 0)

    # :536-600
    def fraction_sfreff(self, ion, part):
        """ion None: get_neutral_fraction_sfreff; 0, 1, 2: get_helium_neutral_fraction_sfreff"""
        sp, net, cu = self.p, self.cool.net, self.cool.units
        redshift, hubble = self.redshift, self.hubble
        a3inv = self.a3inv                                                                                                          # :539 ((1+z)^3: the step's)
        uvbg = self.LocalUVBG                                                                                                       # :547
        physdens = part["Density"] * a3inv                                                                                          # :548
        he = 1 - cr.HYDROGEN_MASSFRAC

        def frac(u, ne):    # GetNeutralFraction / GetHeliumIonFraction (cooling.cpp:147-163)
            rc, uc = physdens * (cu.density_in_phys_cgs / cr.PROTONMASS), u * cu.uu_in_cgs
            if ion is None:
                return net.get_neutral_fraction_phys_cgs(rc, uc, he, uvbg, ne)[0]
            return net.get_helium_ion_phys_cgs(ion, rc, uc, he, uvbg, ne)

        if sp["QuickLymanAlphaProbability"] > 0 or not self.sfreff_on_eeqos(part, a3inv):                                           # :550
            InternalEnergy = part["Entropy"] * cr.entropy_to_u(part["Density"], a3inv)                                              # :552
            return frac(InternalEnergy, part["Ne"]), None                                                                           # :553
        dloga = part["dloga"]                                                                                                       # :559
        dtime = dloga / hubble                                                                                                      # :560
        sfr_data = self.get_sfr_eeqos(part, dtime, uvbg, redshift, a3inv)                                                           # :561
        nh0cold = frac(sp["EgySpecCold"], sfr_data["ne"])                                                                           # :562
        nh0hot = frac(sfr_data["egyhot"], sfr_data["ne"])                                                                           # :563
        return nh0cold * sfr_data["cloudfrac"] + (1 - sfr_data["cloudfrac"]) * nh0hot, sfr_data                                     # :564

    def run(self, what, part):
        """one query of the library for one particle: (outputs dict, ne_internal evaluations, left the table)"""
        net = self.cool.net
        net.evals, net.left_table = 0, False
        part = dict(part)
        if what == "STARFORM":
            out = self.quicklya(part) if self.p["QuickLymanAlphaProbability"] > 0 else self.starformation(part)
        elif what == "EGYEFF":
            out = dict(query=self.get_egyeff(self.redshift, part["Density"], self.GlobalUVBG), flags=part["flags"], decision=0, branch=0)
            out.update(self.last_egyeff)
        elif what == "ON_EEQOS":
            on = self.sfreff_on_eeqos(part, self.a3inv)
            out = dict(egyeff4=part.get("_egyeff4", 0.0), flags=part["flags"], decision=0, branch=(1 if on else 0) | (2 if part.get("_clause4") else 0))
        else:
            q, data = self.fraction_sfreff({"NH0": None, "HE0": 0, "HEP": 1, "HEPP": 2}[what], part)
            out = dict(query=q, egyeff4=part.get("_egyeff4", 0.0), flags=part["flags"], decision=0,
                       branch=(1 if part.get("_on_eeqos") else 0) | (2 if part.get("_clause4") else 0))
            if data is not None:
                out.update(trelax=data["trelax"], tsfr=data["tsfr"], egyhot=data["egyhot"], egycold=data["egycold"], cloudfrac=data["cloudfrac"], ne_eeqos=data["ne"],
                           factorEVP=part["_factorEVP"])
        return out, net.evals, net.left_table
