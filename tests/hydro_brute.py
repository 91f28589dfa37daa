"""All-pairs restatement of hydro_force(): no tree, no oracle, plain numpy.

What the symmetric tree walk of the reference computes (HydroLocalTreeWalk::ngbiter, hydratree2.hpp:253-378, with the HydroPriv ctor
:83-119, the HydroQuery ctor :165-191, the HydroResult ctor :206-210 and HydroOutput::postprocess :134-148; SPH_VelPred and
SPH_EntVarPred, density2.h:89-128; winds_decoupled_hydro, winds.h:60-68) is, per target i, a sum over every gas particle j with

    0 < r2  and  (r2 < Hsml_i^2  or  r2 < Hsml_j^2)  and  DelayTime_j <= 0,

r2 from the minimum-image displacement.  Here that sum is taken over ALL gas particles, so nothing of the node hmax, of cull_node or
of the order of a walk enters: a neighbour whose radius reaches the target from outside the target's own is found because it is in
the table, not because some node's hmax said so.

Per-particle quantities (predicted velocity, entropy variable, drifted densities, pressure, sound speed, the Balsara factor) are
formed in f64 as the reference writes them, with its decisions (the 0.05 Entropy floor, the 1e-6 Density guard) taken on those f64
values.  The one decision per pair, the search test above, is taken on the f64 r2 of the f64 displacement.  The pair terms are then
formed and accumulated in np.longdouble and rounded to f64 once.  Every other branch of a pair (vdotr2 < 0, the viscosity limiter's
fmin, the contrast clamp) is continuous across its switch, so the precision in which it is decided does not matter.

Two sides of a pair are not symmetric in the reference, and are not here:
  - the target's Density and EgyWtDensity are taken as they stand (HydroQuery), the neighbour's drifted by drifts[TimeBinHydro_j];
  - with the EntVarPred cache the target's pressure is PressurePred[pi], made from the DRIFTED density of the target's own bin;
    without the cache it is made from the un-drifted one.  For an active target (drift zero) the two agree.
"""
import numpy as np

from density_brute import GAMMA, KERNELS, LD, dwk_int, min_image

GAMMA_MINUS1 = GAMMA - 1
COUNTERS = ("by_hi_only", "by_hj_only", "by_both", "wrapped", "approaching", "limiter_bites", "limiter_off", "contrast_i", "contrast_j",
            "density_guard", "wind_skipped", "coincident", "f_zero")
SPH_FIELDS = ("Density", "EgyWtDensity", "DhsmlEgyDensityFactor", "DivVel", "CurlVel", "Entropy", "DtEntropy", "HydroAccel", "DelayTime")


def _seg_sum(x, starts, empty):
    """sums of consecutive segments of x, zero for empty ones (density_brute._seg_sum clamps the start of a trailing empty segment
    into the one before it; there every target has itself for a neighbour and no segment is empty, here some are)"""
    s = np.zeros(len(starts), dtype=x.dtype)
    if len(x):
        s[~empty] = np.add.reduceat(x, starts[~empty])
    return s


def kick_arrays(kf):
    """(FgravkickB, gravkicks, hydrokicks, dloga_kick, dloga_for_bin) of a KickFactorData-like record (attributes, tables indexable
    by bin), or all zero for None"""
    if kf is None:
        z = np.zeros(256)
        return 0.0, z, z, z, z
    return (float(kf.FgravkickB),) + tuple(np.array(list(getattr(kf, k)), dtype=np.float64) for k in
                                           ("gravkicks", "hydrokicks", "dloga_kick", "dloga_for_bin"))


def density_pred(density, divvel, dtdrift):
    """SPH_DensityPred, hydratree2.hpp:22-33.  Returns (value, the guard was taken)"""
    pred = density - divvel * density * dtdrift
    guard = ~(pred >= 1e-6 * density)
    return np.where(guard, 1e-6 * density, pred), guard


def pressure_predict(eom, evp):
    """PressurePredict, hydratree2.hpp:48-58"""
    x = evp * eom
    with np.errstate(all="ignore"):
        return np.where(x <= 0, 0.0, np.exp(GAMMA * np.log(np.where(x <= 0, 1.0, x))))


def entvar_pred(entropy, dtentropy, dloga_kick):
    """SPH_EntVarPred, density2.h:115-128"""
    e = entropy + dtentropy * dloga_kick
    e = np.where(e < 0.05 * entropy, 0.05 * entropy, e)
    with np.errstate(all="ignore"):
        return np.where(e <= 0, 0.0, np.exp(1.0 / GAMMA * np.log(np.where(e <= 0, 1.0, e))))


def dwk(ktype, H, r):
    """DensityKernel::dwk(r / H) for support radius H, in the precision of the arguments (as density_brute.kernel_values forms it)"""
    support, sigma = KERNELS[ktype]
    half = support / 2.0
    return sigma * (half / H) ** 3 * half / H * dwk_int(ktype, r / H * half)


def time_factors(atime, hubble):
    """(fac_mu, fac_vsic_fix, hubble_a2) of the HydroPriv ctor, hydratree2.hpp:85-86"""
    return atime ** (3 * GAMMA_MINUS1 / 2) / atime, hubble * atime ** (3 * GAMMA_MINUS1), hubble * atime * atime


def hydro(pos, ptype, mass, hsml, vel, treeacc, gravpm, bins_hydro, bins_grav, sph, evp, params, targets, pi=None, chunk=64):
    """hydro_force() for the gas particles among `targets` (particle indices, any order; non-gas entries give NaN rows).
    `sph`: dict of the by-slot input fields SPH_FIELDS.  `evp`: the EntVarPred cache by slot, or None.  `pi`: slot of each particle
    (None: the gas particles hold slots 0, 1, ... in particle order).  `params`: record with box, kernel, DISPH, contrast, visc,
    atime, hubble, kf (KickFactorData-like or None), drifts (by bin, or None), WindSpeed, WindFreeTravelDensThresh.
    Returns a dict of arrays by position in `targets`; see the module docstring of hydro_cases.py for the counters."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    mass, hsml = np.asarray(mass, dtype=np.float64), np.asarray(hsml, dtype=np.float64)
    treeacc, gravpm = np.asarray(treeacc, dtype=np.float64), np.asarray(gravpm, dtype=np.float64)
    ptype, targets = np.asarray(ptype), np.asarray(targets, dtype=np.int64)
    bh, bg = np.asarray(bins_hydro).astype(np.int64), np.asarray(bins_grav).astype(np.int64)
    n = len(pos)
    box, ktype, DISPH, contrast = float(params.box), params.kernel, bool(params.DISPH), float(params.contrast)
    fac_mu, fac_vsic_fix, hubble_a2 = time_factors(params.atime, params.hubble)
    FgravkickB, gravkicks, hydrokicks, dloga_kick, dloga_for_bin = kick_arrays(params.kf)
    drifts = np.zeros(256) if params.drifts is None else np.asarray(params.drifts, dtype=np.float64)
    gas = np.flatnonzero(ptype == 0)
    if pi is None:
        pi = np.zeros(n, dtype=np.int64)
        pi[gas] = np.arange(len(gas))
    slot = np.asarray(pi, dtype=np.int64)[gas]
    S = {k: np.asarray(sph[k], dtype=np.float64)[slot] for k in SPH_FIELDS}          # by position in `gas`
    gbh = bh[gas]
    # ---- per gas particle, f64 ----
    velp = vel[gas] + gravkicks[bg[gas]][:, None] * treeacc[gas] + gravpm[gas] * FgravkickB + hydrokicks[gbh][:, None] * S["HydroAccel"]
    EVP = np.asarray(evp, dtype=np.float64)[slot] if evp is not None else entvar_pred(S["Entropy"], S["DtEntropy"], dloga_kick[gbh])
    eom0 = S["EgyWtDensity"] if DISPH else S["Density"]
    dens_j, guard = density_pred(S["Density"], S["DivVel"], drifts[gbh])
    eom_j, guard2 = density_pred(eom0, S["DivVel"], drifts[gbh])
    guard = guard | guard2
    P_j = pressure_predict(eom_j, EVP)                                                  # PressurePred[pj] where there is a cache
    with np.errstate(all="ignore"):
        cs_j = np.sqrt(GAMMA * P_j / eom_j)
        f2 = np.abs(S["DivVel"]) / (np.abs(S["DivVel"]) + S["CurlVel"] + 0.0001 * cs_j / fac_mu / hsml[gas])
        # the same particle as a target (HydroQuery ctor)
        P_i = P_j if evp is not None else pressure_predict(eom0, EVP)
        cs_i = np.sqrt(GAMMA * P_i / eom0)
        F1 = np.abs(S["DivVel"]) / (np.abs(S["DivVel"]) + S["CurlVel"] + 0.0001 * cs_i / hsml[gas] / fac_mu)
        por2_i = P_i / (eom0 * eom0)
        por2_j = P_j / (eom_j * eom_j)
        rr1 = eom0 / S["Density"]
        rr2 = eom_j / dens_j
    fzero = (S["DivVel"] == 0) & (S["CurlVel"] == 0)
    decoupled = S["DelayTime"] > 0
    clamp1 = clamp2 = np.zeros(len(gas), dtype=bool)
    if not DISPH:
        rr1, rr2 = np.ones(len(gas)), np.ones(len(gas))
    elif contrast < 0:
        rr1, rr2 = np.zeros(len(gas)), np.zeros(len(gas))
    elif contrast > 0:
        clamp1, clamp2 = rr1 > contrast, rr2 > contrast
        rr1, rr2 = np.minimum(rr1, contrast), np.minimum(rr2, contrast)
    gpos, ghs, gmass = pos[gas], hsml[gas], mass[gas]
    where_in_gas = np.full(n, -1, dtype=np.int64)
    where_in_gas[gas] = np.arange(len(gas))

    nt = len(targets)
    out = {"HydroAccel": np.full((nt, 3), np.nan), "DtEntropy": np.full(nt, np.nan), "MaxSignalVel": np.full(nt, np.nan),
           "abs_HydroAccel": np.full((nt, 3), np.nan), "abs_DtEntropy": np.full(nt, np.nan), "npairs": np.zeros(nt, dtype=np.int64)}
    counters = {k: np.zeros(nt, dtype=np.int64) for k in COUNTERS}
    margin = np.inf
    rows = np.flatnonzero(where_in_gas[targets] >= 0)
    for k0 in range(0, len(rows), chunk):
        row = rows[k0:k0 + chunk]
        ig = where_in_gas[targets[row]]                                                 # position of each target in `gas`
        m = len(ig)
        raw = gpos[ig][:, None, :] - gpos[None, :, :]
        d = min_image(raw, box)                                                         # f64; exact for pairs closer than Box / 2
        r2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        hi2, hj2 = (ghs[ig] * ghs[ig])[:, None], (ghs * ghs)[None, :]
        in_i, in_j = r2 < hi2, r2 < hj2
        margin = min(margin, np.abs(r2 / hi2 - 1).min(), np.abs(r2 / hj2 - 1).min())
        notself = np.arange(len(gas))[None, :] != ig[:, None]
        counters["coincident"][row] = ((r2 == 0) & notself).sum(axis=1)
        reach = (r2 > 0) & (in_i | in_j)
        counters["wind_skipped"][row] = (reach & decoupled[None, :]).sum(axis=1)
        acc = reach & ~decoupled[None, :]
        counters["by_hi_only"][row] = (acc & in_i & ~in_j).sum(axis=1)
        counters["by_hj_only"][row] = (acc & ~in_i & in_j).sum(axis=1)
        counters["by_both"][row] = (acc & in_i & in_j).sum(axis=1)
        counters["wrapped"][row] = (acc & np.any(d != raw, axis=2)).sum(axis=1)
        ti, gj = np.nonzero(acc)                                                        # row-major: grouped by target
        cnt = np.bincount(ti, minlength=m)
        starts = np.concatenate(([0], np.cumsum(cnt)[:-1]))
        empty = cnt == 0
        seg = lambda x: _seg_sum(x, starts, empty)                                      # noqa: E731
        isum = lambda b: _seg_sum(b.astype(np.int64), starts, empty)                    # noqa: E731
        gi = ig[ti]
        # ---- per pair, long double ----
        dl = d[ti, gj].astype(LD)
        r2l = (dl * dl).sum(axis=1)
        r = np.sqrt(r2l)
        dwk_i, dwk_j = dwk(ktype, ghs[gi].astype(LD), r), dwk(ktype, ghs[gj].astype(LD), r)
        dws = dwk_i + dwk_j
        mj = gmass[gj].astype(LD)
        dv = velp[gi].astype(LD) - velp[gj].astype(LD)
        vdotr2 = (dl * dv).sum(axis=1) + hubble_a2 * r2l
        csi, csj = cs_i[gi].astype(LD), cs_j[gj].astype(LD)
        vsig = csi + csj
        appr = vdotr2 < 0
        mu = fac_mu * vdotr2 / r
        vsig_v = vsig - 3 * mu
        rho_ij = 0.5 * (S["Density"][gi].astype(LD) + dens_j[gj].astype(LD))
        with np.errstate(all="ignore"):
            visc = 0.25 * params.visc * vsig_v * (-mu) / rho_ij * (F1[gi].astype(LD) + f2[gj].astype(LD))
            dloga = 2 * np.maximum(dloga_for_bin[gbh[gi]], dloga_for_bin[gbh[gj]])
            msum = gmass[gi].astype(LD) + mj
            lim_on = appr & (dloga > 0) & (dws < 0) & (msum > 0)
            cap = 0.5 * fac_vsic_fix * vdotr2 / (0.5 * msum * dws * r * np.where(dloga > 0, dloga, 1).astype(LD))
        bites = lim_on & (cap < visc)
        visc = np.where(appr, np.where(bites, cap, visc), 0)
        hfc_visc = 0.5 * mj * visc * dws / r
        hfc = hfc_visc
        pi_, pj_ = por2_i[gi].astype(LD), por2_j[gj].astype(LD)
        if DISPH:
            ei, ej = EVP[gi].astype(LD), EVP[gj].astype(LD)
            hfc = hfc + mj * (dwk_i * pi_ * ej / ei + dwk_j * pj_ * ei / ej) / r
        hfc = hfc + mj * (pi_ * S["DhsmlEgyDensityFactor"][gi].astype(LD) * dwk_i * rr1[gi].astype(LD)
                          + pj_ * S["DhsmlEgyDensityFactor"][gj].astype(LD) * dwk_j * rr2[gj].astype(LD)) / r
        at = -hfc[:, None] * dl
        et = 0.5 * hfc_visc * vdotr2
        # HydroOutput::postprocess
        post = GAMMA_MINUS1 / (hubble_a2 * S["Density"][ig] ** GAMMA_MINUS1)
        wind = decoupled[ig]
        for k in range(3):
            out["HydroAccel"][row, k] = np.where(wind, 0.0, seg(at[:, k]).astype(np.float64))
            out["abs_HydroAccel"][row, k] = seg(np.abs(at[:, k])).astype(np.float64)
        out["DtEntropy"][row] = np.where(wind, 0.0, seg(et).astype(np.float64) * post)
        out["abs_DtEntropy"][row] = seg(np.abs(et)).astype(np.float64) * post
        ms = cs_i[ig].astype(LD)                                                        # HydroResult ctor: sqrt(GAMMA Pressure / EgyRho)
        if len(ti):
            sig = np.where(appr, np.maximum(vsig, vsig_v), vsig)
            ms[~empty] = np.maximum(ms[~empty], np.maximum.reduceat(sig, starts[~empty]))
        ms = ms.astype(np.float64)
        windspeed = params.WindSpeed * params.atime * fac_mu
        with np.errstate(all="ignore"):
            hsml_c = np.cbrt(params.WindFreeTravelDensThresh / S["Density"][ig]) * params.atime
        out["MaxSignalVel"][row] = np.where(wind, hsml_c * np.maximum(2 * windspeed, ms), ms)
        out["npairs"][row] = cnt
        counters["approaching"][row] = isum(appr)
        counters["limiter_bites"][row] = isum(bites)
        counters["limiter_off"][row] = isum(appr & (dloga == 0))
        counters["contrast_i"][row] = isum(clamp1[gi])
        counters["contrast_j"][row] = isum(clamp2[gj])
        counters["density_guard"][row] = isum(guard[gj])
        counters["f_zero"][row] = isum(fzero[gi] | fzero[gj])
    out["counters"] = counters
    out["margin"] = float(margin)
    return out
