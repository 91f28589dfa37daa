"""Run start-up (csrc/startup.hip): what the reference does between petaio_read_snapshot and the first step.  init()'s check and
initialisation loops work on device-resident records (objects with a data_ptr(): torch uint8 tensors), in the conventions of
snapshot.py; the first smoothing length and the initial entropy work on the context's resident particles; setup_smoothinglengths takes
host views, like density()."""
import collections
import ctypes as C

import numpy as np

from . import capi
from .capi import STARTUP_OMEGA, STARTUP_POSITIONS, STARTUP_HSML, STARTUP_INIT, STARTUP_ALL  # noqa: F401

StartupReport = collections.namedtuple("StartupReport", ["mass_type", "mass_total", "badmass", "noutside", "first_outside", "numzero", "lastzero", "numprob",
                                                         "lastprob", "nbad_delaytime", "first_bad_delaytime"])
SmlStats = collections.namedtuple("SmlStats", ["first", "nrounds", "maxdiff", "nbad_moments", "nbad_hsml"])


class StartupError(capi.ShqError):
    """A condition the reference ends the run on (endrun), with the reference's message."""


def mean_separation(BoxSize, NTotalInit):
    """get_mean_separation: BoxSize / NTotalInit^(1/3) per type, 0 for a type without particles"""
    ms = (C.c_double * 6)()
    nt = (C.c_int64 * 6)(*[int(x) for x in NTotalInit])
    capi.check(capi.hip.shq_startup_mean_separation(ms, float(BoxSize), nt), "startup_mean_separation")
    return np.array(ms[:])


def u_init(InitGasTemp, CMBTemperature, atime, uu_in_cgs, MinEgySpec):
    """(u_init, InitGasTemp used) of setup_smoothinglengths (init.cpp:467-498)"""
    u, T = C.c_double(), C.c_double()
    capi.check(capi.hip.shq_startup_u_init(float(InitGasTemp), float(CMBTemperature), float(atime), float(uu_in_cgs), float(MinEgySpec), C.byref(u), C.byref(T)),
               "startup_u_init")
    return u.value, T.value


def check_omega(mass_type, mass_total, BoxSize, RhoCrit, Omega0, OmegaNu=0.0, MassiveNuLinRespOn=False, raise_on=False):
    """check_omega's end (init.cpp:223-236) from the (all-reduced) sums of startup_particles: (omegas[6], omega, bad)"""
    mt = (C.c_double * 6)(*[float(x) for x in mass_type])
    om, o, bad = (C.c_double * 6)(), C.c_double(), C.c_int()
    capi.check(capi.hip.shq_startup_omega(mt, float(mass_total), float(BoxSize), float(RhoCrit), float(OmegaNu), int(bool(MassiveNuLinRespOn)), float(Omega0), om,
                                          C.byref(o), C.byref(bad)), "startup_omega")
    if bad.value and raise_on:
        raise StartupError("The mass content is Omega0 = %g,but you specified Omega0 = %g in the parameterfile." % (o.value, Omega0))
    return np.array(om[:]), o.value, bool(bad.value)


def meanbar(OmegaBaryon, HubbleParam):
    """check_density_entropy's mean baryon density in internal units of 1 / s^2 / (cm^3 / g) as the reference forms it"""
    m = C.c_double()
    capi.check(capi.hip.shq_startup_meanbar(float(OmegaBaryon), float(HubbleParam), C.byref(m)), "startup_meanbar")
    return m.value


def startup_layout(part_dtype=None, sph_dtype=None, bh_dtype=None):
    """shq_startup_layout of the record dtypes; local_J21 / zreion are taken when the gas slot has them"""
    P = capi.PARTICLE_DTYPE if part_dtype is None else part_dtype
    S = capi.SPH_DTYPE if sph_dtype is None else sph_dtype
    B = capi.BH_DTYPE if bh_dtype is None else bh_dtype
    L = capi.StartupLayout()
    f = P.fields
    L.part_elsize = P.itemsize
    L.off_pos, L.off_mass, L.off_flags, L.off_type, L.off_pi = f["Pos"][1], f["Mass"][1], f["Flags"][1], f["Type"][1], f["PI"][1]
    L.off_hsml, L.off_ti_drift = f["Hsml"][1], f["Ti_drift"][1]
    s = S.fields
    L.sph_elsize = S.itemsize
    for member, field in (("density", "Density"), ("egywtdensity", "EgyWtDensity"), ("entropy", "Entropy"), ("dtentropy", "DtEntropy"),
                          ("maxsignalvel", "MaxSignalVel"), ("hydroaccel", "HydroAccel"), ("dhsmlegydensityfactor", "DhsmlEgyDensityFactor"), ("divvel", "DivVel"),
                          ("curlvel", "CurlVel"), ("sfr", "Sfr"), ("ne", "Ne"), ("delaytime", "DelayTime"), ("metallicity", "Metallicity"), ("metals", "Metals")):
        setattr(L, "sph_off_" + member, s[field][1])
    L.sph_nmetals = int(np.prod(s["Metals"][0].shape))
    L.sph_off_local_j21 = s["local_J21"][1] if "local_J21" in s else capi.NOFIELD
    L.sph_off_zreion = s["zreion"][1] if "zreion" in s else capi.NOFIELD
    b = B.fields
    L.bh_elsize, L.bh_off_mass, L.bh_off_dfaccel, L.bh_off_dragaccel = B.itemsize, b["Mass"][1], b["DFAccel"][1], b["DragAccel"][1]
    L.part_dtype, L.sph_dtype = P, S
    return L


def startup_params(BoxSize, MassTable=(0,) * 6, MeanSeparation=(0,) * 6, Ti_Current=0, generations=1, RestartSnapNum=-1, init_reion=False):
    p = capi.StartupParams()
    p.BoxSize, p.Ti_Current, p.generations, p.RestartSnapNum, p.init_reion = float(BoxSize), int(Ti_Current), int(generations), int(RestartSnapNum), int(bool(init_reion))
    for t in range(6):
        p.MassTable[t], p.MeanSeparation[t] = float(MassTable[t]), float(MeanSeparation[t])
    return p


def _ptr(d):
    return None if d is None else d.data_ptr()


def _record(d, i, dtype):
    return d[int(i) * dtype.itemsize:(int(i) + 1) * dtype.itemsize].cpu().numpy().view(dtype)[0]


def startup_particles(ctx, layout, d_parts, numpart, d_sph, nsph, d_bh, nbh, params, which=STARTUP_ALL, raise_on=False):
    """shq_startup_particles: the loops of `which` in one pass over the records; returns a StartupReport.  With raise_on the conditions the
    reference ends the run on raise StartupError with its message (the records have been processed all the same)."""
    rep = capi.StartupReport()
    capi.check(capi.hip.shq_startup_particles(ctx.h, C.byref(layout), _ptr(d_parts), int(numpart), _ptr(d_sph), int(nsph), _ptr(d_bh), int(nbh), C.byref(params),
                                              int(which), C.byref(rep)), "startup_particles")
    r = StartupReport(np.array(rep.mass_type[:]), rep.mass_total, rep.badmass, rep.noutside, rep.first_outside, rep.numzero, rep.lastzero, rep.numprob, rep.lastprob,
                      rep.nbad_delaytime, rep.first_bad_delaytime)
    if raise_on:
        if r.noutside:
            pos = _record(d_parts, r.first_outside, layout.part_dtype)["Pos"]
            raise StartupError("Particle %d is outside the box (L=%g) at (%g %g %g)" % (r.first_outside, params.BoxSize, pos[0], pos[1], pos[2]))
        if r.numzero > 1:
            pos = _record(d_parts, r.lastzero, layout.part_dtype)["Pos"]
            raise StartupError("Particle positions contain %d zeros at particle %d. Pos %g %g %g. Likely write corruption!" % (r.numzero, r.lastzero, pos[0], pos[1], pos[2]))
        if r.nbad_delaytime:
            rec = _record(d_parts, r.first_bad_delaytime, layout.part_dtype)
            delay = _record(d_sph, rec["PI"], layout.sph_dtype)["DelayTime"]
            value = "" if np.isfinite(delay) else "%g " % delay    # initial-conditions mode has overwritten it with 0 (init.cpp:170)
            raise StartupError("Bad DelayTime %sfor part %d id %d" % (value, r.first_bad_delaytime, rec["ID"]))
    return r


def check_density_entropy(ctx, layout, d_sph, nsph, meanbar, MinEgySpec, atime):
    """shq_startup_check_density_entropy over the gas slot array; returns `bad`, the densities replaced"""
    bad = C.c_int64()
    capi.check(capi.hip.shq_startup_check_density_entropy(ctx.h, C.byref(layout), _ptr(d_sph), int(nsph), float(meanbar), float(MinEgySpec), float(atime),
                                                          C.byref(bad)), "startup_check_density_entropy")
    return bad.value


def set_init_hsml_device(ctx, numpart, MeanGasSeparation, DesNumNgb, want_nodes=True, device="cuda:0"):
    """shq_set_init_hsml on the `numpart` resident particles and the current tree; returns the node each climb ended on (numpy int32, see
    the header for the numbering) or None.  Raises ShqError on the reference's "Bad tree moments" / "Bad hsml guess" conditions; the
    smoothing lengths are written all the same, and the exception carries the nodes as `.nodes`."""
    import torch
    n = int(numpart)
    nodes = torch.full((max(n, 1),), -2, dtype=torch.int32, device=device) if want_nodes else None
    try:
        capi.check(capi.hip.shq_set_init_hsml(ctx.h, float(MeanGasSeparation), float(DesNumNgb), _ptr(nodes)), "set_init_hsml")
    except capi.ShqError as e:
        e.nodes = None if nodes is None else nodes.cpu().numpy()[:n]
        raise
    return None if nodes is None else nodes.cpu().numpy()[:n]


def init_entropy(ctx, u_init, a3, from_egywt=False):
    """shq_init_entropy: Entropy of the resident gas from u_init and Density (or EgyWtDensity)"""
    capi.check(capi.hip.shq_init_entropy(ctx.h, float(u_init), float(a3), int(bool(from_egywt))), "init_entropy")


def setup_smoothinglengths(ctx, RestartSnapNum, pman, SphP, BhP, density_params, MeanGasSeparation, u_init, atime, DensityIndependentSphOn, raise_on=False):
    """setup_smoothinglengths(RestartSnapNum, ...), init.cpp:458-521: returns at once (None) on a restart; else SmlStats(first density
    pass, number of entropy rounds, maxdiff of each round that was followed by the reduction, particles that met set_init_hsml's
    "Bad tree moments" / "Bad hsml guess").  With raise_on those two raise StartupError after the records have been written."""
    if RestartSnapNum >= 0:
        return None
    p = capi.StartupSmlParams()
    p.density = density_params
    p.MeanGasSeparation, p.u_init, p.atime, p.DensityIndependentSphOn = float(MeanGasSeparation), float(u_init), float(atime), int(bool(DensityIndependentSphOn))
    st = capi.StartupSmlStats()
    pv, sv = pman.view(), capi.sph_view(SphP)
    bv = capi.bh_view(BhP) if BhP is not None and len(BhP) else None
    capi.check(capi.hip.shq_setup_smoothinglengths(ctx.h, C.byref(pv), C.byref(sv), None if bv is None else C.byref(bv), C.byref(p), C.byref(st)),
               "setup_smoothinglengths")
    if raise_on and st.nbad_moments:
        raise StartupError("Bad tree moments: %d particles ended on a node longer than the box or lighter than themselves" % st.nbad_moments)
    if raise_on and st.nbad_hsml:
        raise StartupError("Bad hsml guess: %d particles with Hsml <= 0" % st.nbad_hsml)
    return SmlStats(st.first, st.nrounds, np.array(st.maxdiff[:st.nmaxdiff]), st.nbad_moments, st.nbad_hsml)
