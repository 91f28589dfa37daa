"""A particle load whose PM problem is two-dimensional, and its reference at any mesh size (pure numpy).

Particles sit on lines parallel to an integer direction d that has a component +-1, one particle per step of d, N per line (the
line closes on itself in the periodic box).  With BoxSize = Nmesh a cell is 1.0; line bases are multiples of 2^-10 and masses
multiples of 1/16, so every coordinate, CIC weight and fixed-point deposit value is exact.  The deposit is then exactly invariant
under a shift by d.  Call r the axis with d[r] = 1 (d and -d span the same lines) and p < q the other two, a = d[p], b = d[q]:

    rho(X) = f(X_p - a X_r, X_q - b X_r),      phi(X) = g(X_p - a X_r, X_q - b X_r)

The unscaled 3-D spectrum of rho is N fhat(kp, kq) on the plane kr = -(a kp + b kq) (mod N) and zero elsewhere, so with the
project's unscaled transform pair

    ghat(kp, kq) = N fhat(kp, kq) T[k2] Green(kp, kq, fold(-(a kp + b kq))),      g = N^2 ifft2(ghat)

with Green = potential_transfer as cpu_ops.CpuOps.green states it, fold into (-N/2, N/2], and T the optional table of
shq_pm_set_mode_factor by k2 = kp^2 + kq^2 + kr^2.  One N x N fft2 / ifft2 pair (pocketfft) at any N.

Probe particles of mass zero at random 3-D positions deposit nothing and are read out like every other particle: they sample
phi densely.  The readout is the device's arithmetic (CpuOps.readout: 4-point differences with 2/3 and 1/12, then CIC) with
at(X) looked up in g."""
import math

import numpy as np


def frame(d):
    """(r, p, q, a, b) of a direction: r the LAST axis with |d[r]| = 1, d's sign chosen so that d[r] = +1"""
    d = [int(x) for x in d]
    units = [k for k in range(3) if abs(d[k]) == 1]
    assert units, "the direction needs a component +-1"
    r = units[-1]
    d = [x * d[r] for x in d]
    p, q = [k for k in range(3) if k != r]
    return r, p, q, d[p], d[q]


class Sheaf:
    """pos [n, 3], mass [n] (float32-exact doubles), types [n]; rows [:nline_parts] are the lines' particles, line after line
    (line_of[i] = i // N), the rest the probes"""
    def __init__(self, N, d, pos, mass, nlines):
        self.N, self.d, self.pos, self.mass, self.nlines = N, tuple(int(x) for x in d), pos, mass, nlines
        self.nline_parts = nlines * N
        self.nprobes = len(pos) - self.nline_parts
        self.types = np.ones(len(pos), dtype=np.int32)

    def shifted(self, s):
        """every particle moved by the integer vector s (periodic): lines stay lines along d"""
        pos = np.mod(self.pos + np.asarray(s, dtype=np.float64)[None, :], float(self.N))
        return Sheaf(self.N, self.d, pos, self.mass, self.nlines)


def make_sheaf(N, d, nlines, nprobes, seed):
    """nlines lines along d, N particles each, and nprobes massless probes.  The first min(nlines, N) lines start in the cells
    (j, 2 j mod N) of the (p, q) plane at r-cell 0, which makes the support of f cover every u, every v and every b u - a v for
    d = (+-1, +-1, 1) and the axis directions (row_coverage: 100 % of the rows along the three axes, except along an axis
    direction itself); the others start in seeded random cells.  Fractional parts are seeded random multiples of 2^-10, never 0, so
    that each particle puts mass into all eight cells around it."""
    rng = np.random.default_rng(seed)
    r, p, q, a, b = frame(d)
    cu = rng.integers(0, N, nlines)
    cv = rng.integers(0, N, nlines)
    nd = min(nlines, N)
    cu[:nd] = np.arange(nd) % N
    cv[:nd] = (2 * np.arange(nd)) % N
    frac = rng.integers(1, 1024, (nlines, 3)) / 1024.0
    t = np.arange(N, dtype=np.float64)
    pos = np.empty((nlines * N + nprobes, 3))
    lines = pos[: nlines * N].reshape(nlines, N, 3)
    lines[:, :, r] = frac[:, 2][:, None] + t[None, :]
    lines[:, :, p] = np.mod((cu + frac[:, 0])[:, None] + a * t[None, :], float(N))
    lines[:, :, q] = np.mod((cv + frac[:, 1])[:, None] + b * t[None, :], float(N))
    pos[nlines * N:] = rng.random((nprobes, 3)) * N
    mass = np.zeros(len(pos))
    mass[: nlines * N] = np.repeat(rng.integers(16, 48, nlines) / 16.0, N)
    assert np.array_equal(mass, mass.astype(np.float32).astype(np.float64))
    return Sheaf(N, d, pos, mass, nlines)


def deposit_log2scale(total_mass):
    """the library's fixed-point scale rule (shq_particles_upload): 2^(61 - ex), total mass < 2^ex"""
    return 61 - math.frexp(total_mass if total_mass > 0 else 1.0)[1]


def _cic(pos, N):
    ic = np.floor(pos).astype(np.int64)          # BoxSize = Nmesh: position / cell is the position
    return ic % N, pos - ic


def reduced_density(sh):
    """f[u, v] = rho at X_r = 0: the fixed-point CIC deposit (CpuOps.deposit's arithmetic) of the line particles in the r-cells
    N - 1 (their upper corners) and 0 (their lower corners), in mass units"""
    N = sh.N
    r, p, q, a, b = frame(sh.d)
    pos, m = sh.pos[: sh.nline_parts], sh.mass[: sh.nline_parts]
    ic, res = _cic(pos, N)
    scale = 2.0 ** deposit_log2scale(float(sh.mass.sum()))
    f = np.zeros((N, N), dtype=np.int64)
    for off_r, cell in ((0, 0), (1, N - 1)):
        sel = ic[:, r] == cell
        i, e, ms = ic[sel], res[sel], m[sel]
        for c in range(4):
            off = [0, 0, 0]
            off[p], off[q], off[r] = c & 1, c >> 1, off_r
            w = np.ones(len(ms))
            for k in range(3):                   # the weights' product in the device's order: axis 0, 1, 2
                w = w * (e[:, k] if off[k] else (1 - e[:, k]))
            np.add.at(f, ((i[:, p] + off[p]) % N, (i[:, q] + off[q]) % N), np.rint(w * ms * scale).astype(np.int64))
    return f.astype(np.float64) / scale


def _fold(k, N):
    k = np.mod(k, N)
    return np.where(k <= N // 2, k, k - N)


def _modes(N, d):
    """the excited modes: integer (k_p, k_q, k_r) on the N x N grid of fft2(f), each folded into (-N/2, N/2]"""
    r, p, q, a, b = frame(d)
    k1 = _fold(np.arange(N), N)
    kp, kq = np.meshgrid(k1, k1, indexing="ij")
    return kp, kq, _fold(-(a * kp + b * kq), N)


def _invsinc2(k, N):
    """1 / sinc^2(pi k / N), as CpuOps.green's sinc table"""
    tmp = k * np.pi / N
    s = np.where(np.abs(tmp) < 1e-5, 1.0 - tmp**2 / 6 + tmp**4 / 120, np.sin(tmp) / np.where(tmp == 0, 1, tmp))
    return 1.0 / (s * s)


def reduced_potential(sh, Asmth, G, modefac=None):
    """g[u, v]: the potential mesh phi(X) = g[(X_p - a X_r) % N, (X_q - b X_r) % N]"""
    N = sh.N
    kp, kq, kr = _modes(N, sh.d)
    k2 = kp * kp + kq * kq + kr * kr
    asmth2 = ((2 * np.pi) * Asmth / N) ** 2
    tab = _invsinc2(_fold(np.arange(N), N), N)                                  # by mesh index, like the device's table
    f = tab[kp % N] * tab[kq % N] * tab[kr % N]
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = (-G / (np.pi * N)) * np.exp(-k2 * asmth2) / k2 * f * f       # BoxSize = N
    fac[k2 == 0] = 0.0
    if modefac is not None:
        fac = fac * np.asarray(modefac)[k2]
    fhat = np.fft.fft2(reduced_density(sh))
    return (float(N) ** 3) * np.fft.ifft2(fhat * fac).real


def readout(sh, g, rows):
    """CpuOps.readout on the rows `rows` of the sheaf, the potential mesh looked up in g.  Returns (GravPM [len(rows), 3], pot)."""
    N = sh.N
    r, p, q, a, b = frame(sh.d)
    ic, res = _cic(sh.pos[rows], N)
    ffac = -1.0                                   # -(N / BoxSize)
    c1, c2 = 2.0 / 3.0, 1.0 / 12.0
    grav = np.zeros((len(rows), 3))
    pot = np.zeros(len(rows))

    def at(dx, dy, dz):
        X = (ic[:, 0] + dx, ic[:, 1] + dy, ic[:, 2] + dz)
        return g[(X[p] - a * X[r]) % N, (X[q] - b * X[r]) % N]

    for c in range(8):
        o = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
        w = (res[:, 0] if o[0] else 1 - res[:, 0]) * (res[:, 1] if o[1] else 1 - res[:, 1]) * (res[:, 2] if o[2] else 1 - res[:, 2])
        pot += w * at(*o)
        for k in range(3):
            e = [0, 0, 0]
            e[k] = 1
            s1 = at(o[0] + e[0], o[1] + e[1], o[2] + e[2]) - at(o[0] - e[0], o[1] - e[1], o[2] - e[2])
            s2 = at(o[0] + 2 * e[0], o[1] + 2 * e[1], o[2] + 2 * e[2]) - at(o[0] - 2 * e[0], o[1] - 2 * e[1], o[2] - 2 * e[2])
            grav[:, k] += w * (ffac * (c1 * s1 - c2 * s2))
    return grav, pot


def reduced_reference(sh, Asmth, G, modefac=None):
    """GravPM [n, 3] and the PM potential [n] of every particle of the sheaf, lines and probes, for BoxSize = Nmesh.  The
    particles of a line share their residuals and see the same g: the readout of a line's first particle, evaluated once, is the
    readout of all of them to the bit."""
    N = sh.N
    g = reduced_potential(sh, Asmth, G, modefac)
    rows = np.concatenate([np.arange(sh.nlines) * N, np.arange(sh.nline_parts, len(sh.pos))])
    grav, pot = readout(sh, g, rows)
    back = np.concatenate([np.repeat(np.arange(sh.nlines), N), sh.nlines + np.arange(sh.nprobes)])
    return grav[back], pot[back]


def power_sums(sh, size=None):
    """The raw P(k) sums of the density (orc.power_spectrum's binning and sinc weights) over the N^2 excited modes of the FULL
    spectrum, each counted once: the half spectrum's weights 1 (kz = 0, N/2) and 2 (a mode and its mirror image) say the same.
    Returns power [size] and norm = |rho_0|^2.  (kk and nmodes do not depend on the input.)"""
    N = sh.N
    size = N if size is None else size
    kp, kq, kr = _modes(N, sh.d)
    k2 = kp * kp + kq * kq + kr * kr
    dk = float(N) * np.fft.fft2(reduced_density(sh))
    m = dk.real**2 + dk.imag**2

    def invsinc2(k):
        t = k * np.pi / N
        s = np.where(k == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
        return 1.0 / (s * s)

    tab = invsinc2(_fold(np.arange(N), N))
    f = tab[kp % N] * tab[kq % N] * tab[kr % N]
    binsperunit = (size - 1) / np.log(np.sqrt(3) * N / 2.0)
    sel = k2 > 0
    kint = np.floor(binsperunit * np.log(k2[sel].astype(np.float64)) / 2.0).astype(np.int64)
    ok = kint < size
    power = np.bincount(kint[ok], weights=(m[sel] * f[sel] ** 2)[ok], minlength=size)
    return power, float(m[0, 0])


def row_coverage(sh):
    """share of the mesh rows along axis 0, 1, 2 that hold mass, from the support S of f alone.  A row along p holds mass where
    its v = X_q - b X_r has support, one along q where its u has: |V| / N and |U| / N.  A row along r through (X_p, X_q) holds mass
    when some (u, v) of S has X_p = u + a z, X_q = v + b z: with a or b a unit that says b X_p - a X_q = b u - a v, and every
    such value is taken by N rows: |W| / N.  For a = b = 0 (d an axis) the rows along r are S itself, |S| / N^2 - at most
    4 nlines / N^2."""
    N = sh.N
    r, p, q, a, b = frame(sh.d)
    S = reduced_density(sh) != 0
    u, v = np.nonzero(S)
    share = [0.0, 0.0, 0.0]
    share[p] = len(np.unique(v)) / N
    share[q] = len(np.unique(u)) / N
    if a == 0 and b == 0:
        share[r] = len(u) / N**2
    elif abs(a) == 1 or abs(b) == 1:
        share[r] = len(np.unique((b * u - a * v) % N)) / N
    else:
        assert N <= 128, "neither a nor b is a unit: the union over z is taken cell by cell"
        cov = np.zeros((N, N), dtype=bool)
        for z in range(N):
            cov |= np.roll(S, (a * z, b * z), axis=(0, 1))
        share[r] = cov.sum() / N**2
    return share


def mode_factor(N):
    """a smooth non-trivial T[k2] for shq_pm_set_mode_factor: 1 + 0.3 tanh(log |k|), |k| in mesh units; 3 (N/2)^2 + 1 entries"""
    k2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
    return 1.0 + 0.3 * np.tanh(0.5 * np.log(np.maximum(k2, 1e-30)))


# ---- the cases of the GPU tests, here so that the CPU tests can assert their row coverage without a device --------------------
DIAGONALS = ((1, 1, 1), (1, -1, 1))
AXES = ((0, 0, 1), (1, 0, 0))
AXIS_SIZES = (48, 768, 960, 1024)
NPROBES = 1 << 17
MAX_AXIS_PARTICLES = 5_000_000
AXIS_SPARSE_SHARE = 0.01          # 4 MAX_AXIS_PARTICLES / N^3 less the overlaps: 4.3 % at 768, 1.8 % at 1024


def nlines_for(N, d):
    """2 N lines for the diagonal directions (100 % of the rows along every axis).  Along an axis direction d itself the rows that
    hold mass are the lines' own 2 x 2 columns, so 90 % of them takes about 0.6 N^2 lines - N^3 particles: done where that is
    small (0.75 N^2 lines up to MAX_AXIS_PARTICLES: Nmesh 48), and as many lines as MAX_AXIS_PARTICLES allows otherwise (768 and
    up: 6510 ... 4882 lines), where the rows ALONG d stay sparse (axis_rows_sparse) and the other two axes are covered."""
    if not axis_rows_sparse(N, d):
        r, p, q, a, b = frame(d)
        return 3 * N * N // 4 if a == 0 and b == 0 else 2 * N
    return max(4 * N, MAX_AXIS_PARTICLES // N)


def axis_rows_sparse(N, d):
    """d is an axis and 90 % of the rows along it are out of reach: they hold AXIS_SPARSE_SHARE at least"""
    r, p, q, a, b = frame(d)
    return a == 0 and b == 0 and 3 * N**3 // 4 > MAX_AXIS_PARTICLES


def gpu_case(N, d, nprobes=NPROBES):
    """the sheaf of the GPU tests for (Nmesh, direction): one seed per pair"""
    return make_sheaf(N, d, nlines_for(N, d), nprobes, 1000 * N + sum((x % 3) * 3**k for k, x in enumerate(d)))


def compiled_sizes():
    """the mesh sizes with a bespoke transform, asked of the library itself (shq_fft3d_supported through shq_pm_slab_pitch: needs no
    device), so that a size added there is tested without anybody copying a list.  Every n up to 8192 is asked: a mesh of 8192^3
    doubles is 4 TB, beyond any device's memory, so no size that can run is missed."""
    from shenqi_amd import capi
    return [n for n in range(1, 8193) if capi.hip.shq_pm_slab_pitch(n) != 0]


def gpu_cases():
    """(Nmesh, d) of the run on every compiled size"""
    return [(n, d) for n in compiled_sizes() for d in DIAGONALS] + [(n, d) for n in AXIS_SIZES for d in AXES]
