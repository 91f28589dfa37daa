"""Run logs (csrc/stats.hip): the particle loops behind energy.txt, blackholes.txt and the black-hole details file on device-resident
records (objects with a data_ptr(): torch uint8 tensors), in the conventions of startup.py and snapshot.py, and the text of the three
log lines.  The all-reduce between the loops and the lines, and the files, stay with the caller."""
import ctypes as C
import math

import numpy as np

from . import capi

# physconst.h
GRAVITY, SOLAR_MASS, LIGHTCGS, PROTONMASS, THOMPSON, SEC_PER_YEAR = 6.672e-8, 1.989e33, 2.99792458e10, 1.6726e-24, 6.65245e-25, 3.155e7

# struct BHinfo (bhinfo.cpp:12-63), packed, MyFloat a double
BHINFO_DTYPE = np.dtype({
    "names": ["size1", "ID", "Mass", "Mdot", "Density", "minTimeBin", "encounter", "MinPotPos", "MinPot", "BH_Entropy", "BH_SurroundingGasVel",
              "BH_accreted_momentum", "BH_accreted_Mass", "BH_accreted_BHMass", "BH_FeedbackWeightSum", "SPH_SwallowID", "SwallowID", "CountProgs", "Swallowed",
              "Pos", "BH_SurroundingDensity", "BH_SurroundingParticles", "BH_SurroundingVel", "BH_SurroundingRmsVel", "BH_DFAccel", "BH_DragAccel",
              "BH_FullTreeGravAccel", "Velocity", "Mtrack", "Mdyn", "KineticFdbkEnergy", "NumDM", "V1sumDM", "VDisp", "MgasEnc", "KEflag", "a", "size2"],
    "formats": ["<i4", "<u8", "<f8", "<f8", "<f8", "<i4", "<i4", ("<f8", 3), "<f8", "<f8", ("<f8", 3),
                ("<f8", 3), "<f8", "<f8", "<f8", "<u8", "<u8", "<i4", "<i4",
                ("<f8", 3), "<f8", "<f8", ("<f8", 3), "<f8", ("<f8", 3), ("<f8", 3),
                ("<f8", 3), ("<f8", 3), "<f8", "<f8", "<f8", "<f8", ("<f8", 3), "<f8", "<f8", "<i4", "<f8", "<i4"],
    "offsets": [0, 4, 12, 20, 28, 36, 40, 44, 68, 76, 84,
                108, 132, 140, 148, 156, 164, 172, 176,
                180, 204, 212, 220, 244, 252, 276,
                300, 324, 348, 356, 364, 372, 380, 404, 412, 420, 424, 432],
    "itemsize": capi.BHINFO_SIZE,
})


def _ptr(d):
    return None if d is None else d.data_ptr()


def stats_layout(part_dtype=None, sph_dtype=None):
    """shq_stats_layout of the record dtypes; local_J21 / zreion are taken when the gas slot has them"""
    P = capi.PARTICLE_DTYPE if part_dtype is None else part_dtype
    S = capi.SPH_DTYPE if sph_dtype is None else sph_dtype
    L = capi.StatsLayout()
    f, s = P.fields, S.fields
    L.part_elsize = P.itemsize
    L.off_pos, L.off_mass, L.off_type, L.off_pi, L.off_vel, L.off_potential = (f[k][1] for k in ("Pos", "Mass", "Type", "PI", "Vel", "Potential"))
    L.sph_elsize = S.itemsize
    L.sph_off_density, L.sph_off_entropy, L.sph_off_ne = s["Density"][1], s["Entropy"][1], s["Ne"][1]
    L.sph_off_local_j21 = s["local_J21"][1] if "local_J21" in s else capi.NOFIELD
    L.sph_off_zreion = s["zreion"][1] if "zreion" in s else capi.NOFIELD
    return L


def stats_params(Time, want_temperature=True, uvbg_mode=capi.COOL_UVBG_GLOBAL, GlobalUVBG=None, CurrentParticleOffset=(0.0, 0.0, 0.0), J21_coeffs=(0.0,) * 6,
                 ss_greyopac_factor=0.0, ss_fbar_factor=0.0):
    """shq_stats_params; the UVBG members as shq_cooling_step carries them (GlobalUVBG: a capi.CoolingUVBG)"""
    p = capi.StatsParams()
    p.Time, p.want_temperature, p.uvbg_mode = float(Time), int(bool(want_temperature)), int(uvbg_mode)
    if GlobalUVBG is not None:
        p.GlobalUVBG = GlobalUVBG
    for d in range(3):
        p.CurrentParticleOffset[d] = float(CurrentParticleOffset[d])
    for c in range(6):
        p.J21_coeffs[c] = float(J21_coeffs[c])
    p.ss_greyopac_factor, p.ss_fbar_factor = float(ss_greyopac_factor), float(ss_fbar_factor)
    return p


def energy_statistics(ctx, layout, d_parts, numpart, d_sph, nsph, params, deferred_capacity=None):
    """shq_energy_statistics: the loop of compute_global_quantities_of_system over the records of one rank.  Returns (capi.StatsSums, the
    particle indices whose temperature solve did not end capi.COOL_OK, in index order).  A deferred list longer than deferred_capacity
    (default: room for every particle) raises ShqError with status 3; the exception carries the sums as `.sums`."""
    cap = int(numpart) if deferred_capacity is None else int(deferred_capacity)
    deferred = np.zeros(max(cap, 1), dtype=np.int32)
    sums = capi.StatsSums()
    try:
        capi.check(capi.hip.shq_energy_statistics(ctx.h, C.byref(layout), _ptr(d_parts), int(numpart), _ptr(d_sph), int(nsph), C.byref(params), C.byref(sums),
                                                  capi.ptr(deferred), cap), "energy_statistics")
    except capi.ShqError as e:
        e.sums, e.deferred = sums, deferred[:cap]
        raise
    return sums, deferred[:sums.n_deferred].copy()


def stats_finish(summed):
    """shq_stats_finish: rank 0's block of compute_global_quantities_of_system on sums added over the ranks; returns capi.StatsState"""
    state = capi.StatsState()
    capi.check(capi.hip.shq_stats_finish(C.byref(summed), C.byref(state)), "stats_finish")
    return state


def bh_totals(ctx, d_bh, nbh, bh_dtype=None):
    """shq_bh_totals: (the number of slots with SwallowID == -1, the sums of their Mass, Mdot and Mdot / Mass)"""
    B = capi.BH_DTYPE if bh_dtype is None else bh_dtype
    f = B.fields
    num, sums = C.c_int64(), (C.c_double * 3)()
    capi.check(capi.hip.shq_bh_totals(ctx.h, _ptr(d_bh), int(nbh), B.itemsize, f["SwallowID"][1], f["Mass"][1], f["Mdot"][1], C.byref(num), sums), "bh_totals")
    return num.value, np.array(sums[:])


def bh_detail_layout(part_dtype=None, bh_dtype=None):
    """shq_bh_detail_layout of the record dtypes"""
    P = capi.PARTICLE_DTYPE if part_dtype is None else part_dtype
    B = capi.BH_DTYPE if bh_dtype is None else bh_dtype
    L = capi.BhDetailLayout()
    f, b = P.fields, B.fields
    L.part_elsize = P.itemsize
    for member, field in (("pos", "Pos"), ("mass", "Mass"), ("flags", "Flags"), ("type", "Type"), ("pi", "PI"), ("vel", "Vel"),
                          ("fulltreegravaccel", "FullTreeGravAccel"), ("id", "ID")):
        setattr(L, "off_" + member, f[field][1])
    L.bh_elsize = B.itemsize
    for member, field in (("mintimebin", "minTimeBin"), ("encounter", "encounter"), ("mass", "Mass"), ("mdot", "Mdot"), ("density", "Density"), ("mtrack", "Mtrack"),
                          ("kineticfdbkenergy", "KineticFdbkEnergy"), ("vdisp", "VDisp"), ("dfaccel", "DFAccel"), ("df_surroundingvel", "DF_SurroundingVel"),
                          ("df_surroundingrmsvel", "DF_SurroundingRmsVel"), ("df_surroundingdensity", "DF_SurroundingDensity"), ("dragaccel", "DragAccel"),
                          ("swallowid", "SwallowID"), ("minpot", "MinPot"), ("minpotpos", "MinPotPos"), ("countprogs", "CountProgs")):
        setattr(L, "bh_off_" + member, b[field][1])
    return L


def bh_detail_arrays(arrays=None, n_sph_swallowid=0, CurrentParticleOffset=(0.0, 0.0, 0.0)):
    """shq_bh_detail_arrays from a mapping of capi.BH_DETAIL_ARRAYS names to device arrays (a missing or None entry: NULL, its members stay 0)"""
    X = capi.BhDetailArrays()
    arrays = arrays or {}
    for k in arrays:
        if k not in capi.BH_DETAIL_ARRAYS:
            raise ValueError(f"bh_detail_arrays: no array {k}")
    for k in capi.BH_DETAIL_ARRAYS:
        setattr(X, k, _ptr(arrays.get(k)))
    X.n_sph_swallowid = int(n_sph_swallowid)
    for d in range(3):
        X.CurrentParticleOffset[d] = float(CurrentParticleOffset[d])
    X._keep = dict(arrays)
    return X


def bh_details(ctx, layout, d_parts, numpart, d_bh, nbh, arrays, d_active, nactive, atime, d_out=None, device="cuda:0"):
    """shq_bh_details: the BHinfo records of collect_BH_info for the black holes of d_active (device int32; None: particles 0 .. nactive - 1)
    as a structured array of BHINFO_DTYPE.  d_out: device bytes to compose them in (default: allocated here)."""
    import torch
    n = int(nactive)
    if d_out is None:
        d_out = torch.zeros(max(n, 1) * capi.BHINFO_SIZE, dtype=torch.uint8, device=device)
    capi.check(capi.hip.shq_bh_details(ctx.h, C.byref(layout), _ptr(d_parts), int(numpart), _ptr(d_bh), int(nbh), C.byref(arrays), _ptr(d_active), n, float(atime),
                                       _ptr(d_out)), "bh_details")
    return d_out[:n * capi.BHINFO_SIZE].cpu().numpy().view(BHINFO_DTYPE)


# ---- the lines ------------------------------------------------------------------------------------------------------------------------

def _g(x, spec="%g"):
    """C's printf of a double: Python agrees but for a NaN with the sign bit set, which glibc prints as -nan"""
    x = float(x)
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return spec % x


def energy_line(Time, state):
    """the line energy_statistics writes to energy.txt (stats.cpp:383-393) from a capi.StatsState"""
    s = state
    vals = [Time, s.TemperatureComp[0], s.EnergyInt, s.EnergyPot, s.EnergyKin]
    for t in range(6):
        vals += [s.EnergyIntComp[t], s.EnergyPotComp[t], s.EnergyKinComp[t]]
    vals += [s.MassComp[t] for t in range(6)]
    return " ".join(_g(v) for v in vals) + "\n"


def _unit(units, name):
    return float(units[name] if isinstance(units, dict) else getattr(units, name))


def blackholes_line(atime, num, sums, units):
    """the line write_blackhole_txt writes to blackholes.txt (bhinfo.cpp:186-201) from the counts and sums added over the ranks: sums =
    (Mass, Mdot, Mdot / Mass) as shq_bh_totals returns them; units: UnitMass_in_g and UnitTime_in_s, as attributes or keys"""
    total_mass_holes, total_mdot, total_mdoteddington = (float(x) for x in sums)
    UnitMass_in_g, UnitTime_in_s = _unit(units, "UnitMass_in_g"), _unit(units, "UnitTime_in_s")
    # convert to solar masses per yr
    mdot_in_msun_per_year = total_mdot * (UnitMass_in_g / SOLAR_MASS) / (UnitTime_in_s / SEC_PER_YEAR)
    total_mdoteddington *= 1.0 / ((4 * math.pi * GRAVITY * LIGHTCGS * PROTONMASS / (0.1 * LIGHTCGS * LIGHTCGS * THOMPSON)) * UnitTime_in_s)
    return "%s %d %s %s %s %s\n" % (_g(atime), int(num), _g(total_mass_holes), _g(total_mdot), _g(mdot_in_msun_per_year), _g(total_mdoteddington))


def sfr_line(Time, sums, counts, UnitSfr_in_solar_per_year):
    """the line cooling_and_starformation writes to sfr.txt (sfr_eff.cpp:390-415), or None when it writes none (total_sm <= 0).  All
    arguments added over the ranks: sums = (total_sm, totsfrrate, total_sum_mass_stars, total_sum_dtime), of which shq_sfr_result holds
    sum_sm, localsfr and sum_dtime and the star spawning step the mass of the stars made; counts = (total_sum_part, stars spawned +
    converted), the first being shq_sfr_result's sum_sf_part."""
    total_sm, totsfrrate, total_sum_mass_stars, total_sum_dtime = (float(x) for x in sums)
    total_sum_part, tot_new = (int(x) for x in counts)
    if not total_sm > 0:
        return None
    rate = 0.0
    if total_sum_dtime > 0:
        rate = total_sm * total_sum_part / total_sum_dtime
    # convert to solar masses per yr
    rate_in_msunperyear = rate * float(UnitSfr_in_solar_per_year)
    with np.errstate(all="ignore"):
        mean_dtime = float(np.float64(total_sum_dtime) / np.float64(total_sum_part))   # C's double / int64: no exception at 0
    return "%s %s %s %s %s %s %d %d\n" % (_g(Time, "%.12g"), _g(total_sm), _g(totsfrrate), _g(rate_in_msunperyear), _g(total_sum_mass_stars), _g(mean_dtime),
                                          total_sum_part, tot_new)
