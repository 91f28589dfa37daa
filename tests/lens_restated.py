"""A numpy restatement of the lensing potential planes (write_plane, libgadget/plane.cpp:511-614; cutPlaneGaussianGrid and
calculate_lensing_potential, libgadget/lenstools.cpp:168-319; the PM neutrino correction, plane.cpp:355-475), written from their
description for one rank.

The bins decide integer counts, so every binning expression is plain float64 arithmetic in the reference's order (numpy does not
contract a * b + c into an FMA): the counts must match the device's bit for bit.  The transforms are numpy.fft with explicit
normalisation (unscaled forward, unscaled inverse, then / R^2 as the reference does after FFTW's c2r)."""
import numpy as np

LIGHTCGS = 2.99792458e10          # physconst.h
CM_PER_KPC = 3.085678e21
SMOOTH = 1.0                      # cutPlaneGaussianGrid: fixed


def linspace(start, stop, num):
    """lenstools.cpp linspace: step = (stop - start) / (num - 1); result[i] = start + i * step"""
    step = (stop - start) / (num - 1)
    return start + np.arange(num, dtype=np.float64) * step


def _while_add(x, cond, delta):
    """x[cond(x)] += delta until no element satisfies cond: the reference's `while(cond) x += delta`, element by element"""
    x = np.array(x, dtype=np.float64, copy=True)
    while True:
        m = cond(x)
        if not m.any():
            return x
        x[m] += delta


def wrap_position(v, L):
    """grid3d_ngb: while(> L) -= L; while(<= 0) += L, into (0, L]"""
    v = _while_add(v, lambda x: x > L, -L)
    return _while_add(v, lambda x: x <= 0, L)


def find_bin(value, bins, res, L):
    """lenstools.cpp find_bin for an array of values; -1 where the value is dropped"""
    width = bins[res] - bins[0]
    value = np.asarray(value, dtype=np.float64)
    if width <= 0 or res <= 0:
        return np.full(value.shape, -1, dtype=np.int64)
    rel = value - bins[0]
    rel = _while_add(rel, lambda x: x < 0, L)
    rel = _while_add(rel, lambda x: x >= L, -L)
    out = np.full(value.shape, -1, dtype=np.int64)
    ok = rel < width
    idx = np.floor(rel[ok] / width * res)
    good = (idx >= 0) & (idx < res)
    sel = np.flatnonzero(ok)
    out[sel[good]] = idx[good].astype(np.int64)
    return out


def default_cuts(BoxSize, Thickness):
    """write_plane (plane.cpp:519-530): Thickness <= 0 -> BoxSize; no cut points -> (0.5 + i) Thickness, i < (size_t)(BoxSize / Thickness)"""
    th = BoxSize if Thickness <= 0 else Thickness
    return th, [(.5 + i) * th for i in range(int(BoxSize / th))]


def is_active(flags, types, exclude_type2):
    """lenstools_particle_is_active: not Swallowed (flag bit 1), not Type 2 under hybrid_nu_tracer; IsGarbage is not looked at"""
    act = (np.asarray(flags, np.uint8) & 2) == 0
    if exclude_type2:
        act &= np.asarray(types) != 2
    return act


def count_plane(pos, flags, types, exclude_type2, BoxSize, offset, normal, center, thickness, R):
    """grid3d_ngb + projectDensity for one (cut, normal): uint32 counts [R][R] in the plane layout
    (normal 0 -> [y][z], 1 -> [x][z], 2 -> [x][y])"""
    L = BoxSize
    act = is_active(flags, types, exclude_type2)
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)[act]
    idx = []
    for d in range(3):
        v = wrap_position(p[:, d] - offset[d], L)
        if d == normal:
            idx.append(find_bin(v, linspace(center - thickness / 2, center + thickness / 2, 2), 1, L))
        else:
            idx.append(find_bin(v, linspace(0.0, 0.0 + L, R + 1), R, L))
    keep = (idx[0] >= 0) & (idx[1] >= 0) & (idx[2] >= 0)
    lo, hi = [d for d in range(3) if d != normal]
    flat = idx[lo][keep] * R + idx[hi][keep]
    return np.bincount(flat, minlength=R * R).astype(np.uint32).reshape(R, R)


def l_squared(R):
    """calculate_lensing_potential's multipoles over the r2c half plane [R][R/2 + 1], l2[0][0] = 1"""
    i = np.arange(R, dtype=np.float64)
    lx = np.where(np.arange(R) < R // 2, i, -(R - i)) / R
    ly = np.arange(R // 2 + 1, dtype=np.float64) / R
    l2 = lx[:, None] * lx[:, None] + ly[None, :] * ly[None, :]
    l2[0, 0] = 1.0
    return l2


def filter_factor(R, b0, b1, chi, smooth=SMOOTH):
    """the Poisson and Gaussian factor that multiplies each mode of the half plane (the DC mode is zeroed separately)"""
    l2 = l_squared(R)
    factor = -2.0 * (b0 * b1 / (chi * chi)) / (l2 * 4 * np.pi * np.pi)
    return factor * np.exp(-0.5 * ((2.0 * np.pi * smooth) * (2.0 * np.pi * smooth)) * l2)


def lensing_potential(density, b0, b1, chi, smooth=SMOOTH):
    """calculate_lensing_potential: r2c, DC to zero, the filter, c2r, / R^2"""
    R = density.shape[0]
    F = np.fft.rfft2(density, norm="backward")          # unscaled, as FFTW's r2c
    F[0, 0] = 0.0
    F = F * filter_factor(R, b0, b1, chi, smooth)
    out = np.fft.irfft2(F, s=(R, R), norm="forward")     # unscaled, as FFTW's c2r
    return out / (R * R)


def cosmo_normalization(HubbleParam, omega_source):
    H0 = 100 * HubbleParam * 3.2407793e-20
    return 1.5 * H0 ** 2 * omega_source / LIGHTCGS ** 2


def density_normalization(thickness, chi, HubbleParam, atime):
    return thickness * chi * (CM_PER_KPC / HubbleParam) ** 2 / atime


def norm_factor(num_particles_tot, BoxSize, R, thickness, normal):
    """cutPlaneGaussianGrid's 1 / num_particles_tot * L^3 / (b0 b1 b2), the bin sizes in axis order"""
    b = [BoxSize / R] * 3
    b[normal] = thickness / 1
    return 1. / num_particles_tot * (BoxSize ** 3 / (b[0] * b[1] * b[2]))


def particle_plane(counts, p, c, normal):
    """cutPlaneGaussianGrid from the counts: (potential [R][R], num_particles_plane); p["Thickness"] is the effective one"""
    R = counts.shape[0]
    npl = int(counts.sum(dtype=np.int64))
    if npl == 0:
        return np.zeros((R, R)), 0
    dens = counts.astype(np.float64) * norm_factor(c["num_particles_tot"], p["BoxSize"], R, p["Thickness"], normal)
    pot = lensing_potential(dens, p["BoxSize"] / R, p["BoxSize"] / R, c["comoving_distance"])
    s = cosmo_normalization(c["HubbleParam"], c["omega_source"]) * density_normalization(p["Thickness"], c["comoving_distance"],
                                                                                         c["HubbleParam"], c["atime"])
    return pot * s, npl


# ---- the PM neutrino correction --------------------------------------------------------------


def plane_wrap_position(x, L):
    """plane.cpp plane_wrap_position: into [0, L)"""
    while x < 0:
        x += L
    while x >= L:
        x -= L
    return x


def interval_overlap(a0, a1, b0, b1):
    lo = a0 if a0 > b0 else b0
    hi = a1 if a1 < b1 else b1
    return hi - lo if hi > lo else 0.0


def slab_overlap(cell_start, cellsize, center, thickness, L):
    """plane_periodic_slab_overlap"""
    if thickness >= L:
        return cellsize
    c = plane_wrap_position(center, L)
    slab_start = c - 0.5 * thickness
    slab_end = slab_start + thickness
    cell_end = cell_start + cellsize
    overlap = 0.0
    for shift in (-1, 0, 1):
        offset = shift * L
        overlap += interval_overlap(cell_start, cell_end, slab_start + offset, slab_end + offset)
    return overlap


def overlap_table(N, L, center, thickness):
    cellsize = L / N
    return np.array([slab_overlap(k * cellsize, cellsize, center, thickness, L) for k in range(N)])


def project_correction(real, x0, N, inv_fft_norm, mean_mass_cell, L, normal, center, thickness):
    """cutPlanePMNeutrinoCorrection's projection of the rank's x-slab real [nx][N][N]: the [N][N] plane indexed
    [global[(normal + 1) % 3]][global[(normal + 2) % 3]] (for normal 1: [z][x], the transpose of the particle plane's [x][z])"""
    real = np.asarray(real, dtype=np.float64)
    nx = real.shape[0]
    w = overlap_table(N, L, center, thickness)
    delta = real * inv_fft_norm / mean_mass_cell
    shape = [1, 1, 1]
    shape[normal] = -1
    wk = (w[x0:x0 + nx] if normal == 0 else w).reshape(shape)
    contrib = np.where(wk > 0, delta * wk / thickness, 0.0)
    full = np.zeros((N, N, N))
    full[x0:x0 + nx] = contrib
    s = full.sum(axis=normal)          # normal 0: [y][z]; 1: [x][z]; 2: [x][y]
    return s.T.copy() if normal == 1 else s


def correction_plane(nu, p, c, normal, center):
    """the correction's potential at Nmesh [N][N]; p["Thickness"] is the effective one"""
    N = nu["Nmesh"]
    L = p["BoxSize"]
    th = p["Thickness"]
    dens = project_correction(nu["real"], nu["x0"], N, nu["inv_fft_norm"], nu["mean_mass_cell"], L, normal, center, th)
    cellsize = L / N
    pot = lensing_potential(dens, cellsize, cellsize, c["comoving_distance"])
    return pot * (cosmo_normalization(c["HubbleParam"], c["omega_source"]) *
                  density_normalization(th, c["comoving_distance"], c["HubbleParam"], c["atime"]))


def bilinear_add(dst, src):
    """plane_add_periodic_bilinear: src (src_n^2) interpolated onto dst (dst_n^2) and added, in place"""
    dst_n, src_n = dst.shape[0], src.shape[0]
    x = ((np.arange(dst_n) + 0.5) * src_n / dst_n) - 0.5
    i0 = np.floor(x).astype(np.int64)
    t = x - i0
    i0 = np.mod(i0, src_n)
    i1 = (i0 + 1) % src_n
    tx, ty = t[:, None], t[None, :]
    v00, v10 = src[i0][:, i0], src[i1][:, i0]
    v01, v11 = src[i0][:, i1], src[i1][:, i1]
    dst += (1 - tx) * (1 - ty) * v00 + tx * (1 - ty) * v10 + (1 - tx) * ty * v01 + tx * ty * v11
    return dst


# ---- the whole call ---------------------------------------------------------------------------


def lens_planes(pos, flags, types, p, c, nu=None):
    """shq_lens_planes for one rank.  p: BoxSize, Resolution, Normals, CutPoints (empty or None: the default list), Thickness (<= 0:
    BoxSize), CurrentParticleOffset, exclude_type2.  c: atime, comoving_distance, HubbleParam, omega_source, num_particles_tot.
    nu: None or Nmesh, x0, real [nx][Nmesh][Nmesh], inv_fft_norm, mean_mass_cell.
    Returns (planes [ncuts][nnormals][R][R], num_particles_plane [ncuts][nnormals], counts [ncuts][nnormals][R][R] uint32)."""
    L, R = p["BoxSize"], p["Resolution"]
    th, dcuts = default_cuts(L, p.get("Thickness", 0.0))
    cp = p.get("CutPoints")
    cuts = list(cp) if cp is not None and len(cp) else dcuts
    pp = dict(p, Thickness=th)
    normals = list(p["Normals"])
    planes = np.zeros((len(cuts), len(normals), R, R))
    counts = np.zeros((len(cuts), len(normals), R, R), dtype=np.uint32)
    npl = np.zeros((len(cuts), len(normals)), dtype=np.int64)
    off = p.get("CurrentParticleOffset", (0.0, 0.0, 0.0))
    for i, center in enumerate(cuts):
        for j, normal in enumerate(normals):
            cnt = count_plane(pos, flags, types, p.get("exclude_type2", 0), L, off, normal, center, th, R)
            pot, n = particle_plane(cnt, pp, c, normal)
            if nu is not None:
                bilinear_add(pot, correction_plane(nu, pp, c, normal, center))
            planes[i, j], counts[i, j], npl[i, j] = pot, cnt, n
    return planes, npl, counts
