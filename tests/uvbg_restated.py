"""A numpy restatement of calculate_uvbg + petapm_reion (libgadget/uvbg.cpp, petapm.cpp) for one rank, the parity yardstick of
shq_uvbg_calculate.  The reference's float steps are emulated with np.float32; its libm calls (sinf / cosf / powf / pow) go to glibc
through ctypes.  The deposit is the reference's double CIC (the library deposits in fixed point: the grids agree to rounding)."""
import ctypes as C
import math

import numpy as np

_libm = C.CDLL("libm.so.6")
for _f in ("sinf", "cosf"):
    getattr(_libm, _f).argtypes = [C.c_float]
    getattr(_libm, _f).restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]
_libm.powf.restype = C.c_float
_libm.pow.argtypes = [C.c_double, C.c_double]
_libm.pow.restype = C.c_double

# physconst.h
SOLAR_MASS = 1.989e33
PLANCK = 6.6262e-27
PROTONMASS = 1.6726e-24
SEC_PER_YEAR = 3.155e7
HYDROGEN_MASSFRAC = 0.76
FLOAT_REL_TOL = np.float32(1e-5)      # uvbg.cpp:29
MAX_R_ITERATIONS = 10000              # petapm.cpp:527


def filter_table(filter_type, N, BoxSize, R):
    """filter_pm (uvbg.cpp:218-250) per integer k2 = 0 .. 3 (N/2)^2, with glibc's sinf / cosf / powf / pow"""
    out = np.empty(3 * (N // 2) ** 2 + 1)
    for k2 in range(out.size):
        k_mag = math.sqrt(k2) * (2 * math.pi / N) * (N / BoxSize)        # uvbg.cpp:221
        kR = k_mag * R                                                     # :223
        f = 1.0
        if filter_type == 0:                                               # :226-231
            if kR > 1e-4:
                kf = C.c_float(kR).value
                a = np.float32(_libm.sinf(kf)) / np.float32(_libm.powf(kf, 3.0))
                b = np.float32(_libm.cosf(kf)) / np.float32(_libm.powf(kf, 2.0))
                f = 3.0 * float(np.float32(a - b))
        elif filter_type == 1:                                             # :234-239
            kR *= 0.413566994
            if kR > 1:
                f = 0.0
        elif filter_type == 2:                                             # :242-245
            kR *= 0.643
            f = _libm.pow(math.e, (-kR * kR / 2.0))
        else:
            raise ValueError(filter_type)
        out[k2] = f
    return out


def radius_schedule(Rmax, Rmin, Rdelta, BoxSize, CellSize):
    """petapm_reion_c2r's radius loop (petapm.cpp:536-606): the filter radii in order, the last one the unfiltered cell size"""
    R = min(Rmax, BoxSize)                                                 # :537
    radii, last, count = [], False, 0
    while not last:
        count += 1
        if R / Rdelta < Rmin or R / Rdelta < CellSize or count > MAX_R_ITERATIONS:    # :548
            last = True
            R = CellSize
        radii.append(R)
        R = R / Rdelta                                                     # :604
    return radii


def init_particle_uvbg(types, fesc, use_sfr, Norm, Scaling, UnitMass_in_g, HubbleParam):
    """init_particle_uvbg (uvbg.cpp:474-507): the transformed escape fractions (local_J21 = 0 is the readout's starting value)"""
    conv = UnitMass_in_g / SOLAR_MASS / 1e10 / HubbleParam
    out = fesc.copy()
    sel = ((types == 4) | ((types == 0) & bool(use_sfr))) & (fesc != 0)
    for i in np.flatnonzero(sel):
        t = Norm * _libm.pow(fesc[i] * conv, Scaling)
        if t > 1:
            t = 1.0
        if t < 0:
            raise ValueError("negative escape fraction?")
        out[i] = t
    return out


def _cic(pos, N, cell):
    """pm_iterate_one (petapm.cpp:1133-1189) on the periodic mesh: per particle its 8 (cell index, weight) pairs in connection order"""
    tmp = pos / cell
    ic = np.floor(tmp)
    res = tmp - ic
    ic = ic.astype(np.int64) % N
    idx, wts = [], []
    for c in range(8):
        w = np.ones(len(pos))
        lin = np.zeros(len(pos), dtype=np.int64)
        for k in range(3):
            off = (c >> k) & 1
            lin = lin * N + (ic[:, k] + off) % N
            w = w * (res[:, k] if off else (1 - res[:, k]))
        idx.append(lin)
        wts.append(w)
    return idx, wts


def _deposit(idx, wts, value, sel, N):
    mesh = np.zeros(N ** 3)
    for lin, w in zip(idx, wts):
        mesh += np.bincount(lin[sel], weights=(w * value)[sel], minlength=N ** 3)
    return mesh.reshape(N, N, N)


def calculate_uvbg(p, cp, pos, mass, types, fesc, sfr, local_J21, zreion, near_rel=1e-12):
    """p: dict of UVBGParams + BoxSize; cp: dict Time, Omega0, OmegaBaryon, RhoCrit, HubbleParam, hubble, Unit*.  Returns a dict with
    J21 / xHI (float32 [N]^3), the two global xHI, nradii, fesc / local_J21 / zreion after the call, the radii, and `near`: cells whose
    f_coll_stars came within near_rel (relative) of the ionisation threshold at some radius"""
    N, L = p["UVBGdim"], p["BoxSize"]
    use_sfr = bool(p["ReionUseParticleSFR"])
    cell = L / N                                                           # petapm.cpp:205
    mass = np.asarray(mass, dtype=np.float32).astype(np.float64)
    fesc = init_particle_uvbg(types, fesc, use_sfr, p["EscapeFractionNorm"], p["EscapeFractionScaling"], cp["UnitMass_in_g"],
                              cp["HubbleParam"])
    idx, wts = _cic(pos, N, cell)
    # put_particle_to_mesh / put_star_to_mesh / put_sfr_to_mesh (petapm.cpp:1304-1328): weight * Mass [* fesc]
    fields = [_deposit(idx, wts, mass, np.ones(len(pos), bool), N)]
    star = np.zeros(N ** 3)
    for lin, w in zip(idx, wts):
        s = types == 4
        star += np.bincount(lin[s], weights=(w * mass * fesc)[s], minlength=N ** 3)
    fields.append(star.reshape(N, N, N))
    if use_sfr:
        sf = np.zeros(N ** 3)
        for lin, w in zip(idx, wts):
            s = types == 0
            sf += np.bincount(lin[s], weights=(w * sfr * fesc)[s], minlength=N ** 3)
        fields.append(sf.reshape(N, N, N))
    ncell = N * N * N                                                      # divide_by_ncell's int (uvbg.cpp:211-215)
    spectra = [np.fft.rfftn(f) / ncell for f in fields]
    k1 = np.fft.fftfreq(N, 1.0 / N).astype(np.int64)
    k2 = (k1[:, None, None] ** 2 + k1[None, :, None] ** 2 + np.arange(N // 2 + 1)[None, None, :] ** 2)

    # reion_loop_pm's constants (uvbg.cpp:336-370)
    redshift = 1.0 / cp["Time"] - 1.
    Y_He = 1.0 - HYDROGEN_MASSFRAC
    BaryonFrac = cp["OmegaBaryon"] / cp["Omega0"]
    ReionEfficiency = 1.0 / BaryonFrac * p["ReionNionPhotPerBary"] / (1.0 - 0.75 * Y_He)
    tot_n_cells = float(N * N * N)
    pixel_volume = cell * cell * cell
    deltax_conv_factor = tot_n_cells / (cp["RhoCrit"] * cp["Omega0"] * L * L * L)
    hubble_time = 1 / (cp["hubble"] * cp["HubbleParam"])
    OmegaM, RhoCrit = cp["Omega0"], cp["RhoCrit"]

    J21 = np.zeros((N, N, N), np.float32)
    xHI = np.ones((N, N, N), np.float32)
    near = np.zeros((N, N, N), bool)
    radii = radius_schedule(p["ReionRBubbleMax"], p["ReionRBubbleMin"], p["ReionDeltaRFactor"], L, cell)
    thr = 1.0 / ReionEfficiency
    for r, R in enumerate(radii):
        last = r == len(radii) - 1
        if last:
            T = np.ones_like(k2, dtype=np.float64)
        else:
            T = filter_table(p["ReionFilterType"], N, L, R)[k2]
        real = [np.fft.irfftn(s * T, s=(N, N, N), norm="forward") for s in spectra]      # petapm_fft_c2r, unscaled
        mass_real = np.maximum(real[0], 0.0)
        star_real = np.maximum(real[1], 0.0)
        if p["RtoMFilterType"] == 0:                                       # RtoM, uvbg.cpp:158-176
            RtoM = (4.0 / 3.0) * math.pi * _libm.pow(R, 3) * (OmegaM * RhoCrit)
        else:
            RtoM = _libm.pow(2 * math.pi, 1.5) * OmegaM * RhoCrit * _libm.pow(R, 3)
        J21_aux_constant = ((1.0 + redshift) * (1.0 + redshift) / (4.0 * math.pi) * p["AlphaUV"] * PLANCK * 1e21 * R
                            * cp["UnitLength_in_cm"] * p["ReionNionPhotPerBary"] / PROTONMASS * cp["UnitMass_in_g"]
                            / _libm.pow(cp["UnitLength_in_cm"], 3) / cp["UnitTime_in_s"])
        with np.errstate(divide="ignore", invalid="ignore"):
            density_over_mean = mass_real * deltax_conv_factor
            f_coll_stars = star_real / (RtoM * density_over_mean) * (4.0 / 3.0) * math.pi * R * R * R / pixel_volume
        if use_sfr:
            sfr_real = np.maximum(real[2], 0.0)
            sfr_density = sfr_real / pixel_volume / (cp["UnitMass_in_g"] / SOLAR_MASS) * (cp["UnitTime_in_s"] / SEC_PER_YEAR)
        else:
            sfr_density = star_real / (p["ReionSFRTimescale"] * hubble_time) / pixel_volume
        J21_aux = (sfr_density * J21_aux_constant).astype(np.float32)
        near |= np.abs(f_coll_stars - thr) <= near_rel * thr
        ion = f_coll_stars > thr
        first = ion & (xHI > FLOAT_REL_TOL)
        J21[first] = J21_aux[first]
        xHI[ion] = 0.0
        if last:
            part = ~ion & (xHI > FLOAT_REL_TOL)
            xHI[part] = (1.0 - f_coll_stars[part] * ReionEfficiency).astype(np.float32)
            d = deltax_conv_factor * mass_real
            vol = float(xHI.astype(np.float64).sum()) / (N ** 3)
            mw = float((xHI.astype(np.float64) * d).sum()) / float(d.sum())

    # readout_J21 (uvbg.cpp:461-472) over the 8 cells, zero weights included
    lj = local_J21.copy()
    zr = zreion.copy()
    gas = types == 0
    lj[gas] = 0.0
    Jf = J21.reshape(-1).astype(np.float64)
    for lin in idx:
        v = Jf[lin]
        up = gas & (v > lj)
        lj[up] = v[up]
        zr[up & (zr == -1)] = 1 / cp["Time"] - 1
    return dict(J21=J21, xHI=xHI, vol=vol, mass=mw, nradii=len(radii), radii=radii, fesc=fesc, local_J21=lj, zreion=zr, near=near,
                cells=np.stack(idx, axis=1))
