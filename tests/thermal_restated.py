"""A plain Python / numpy restatement of the thermal velocities (add_thermal_speeds, init_rng and init_thermalvel of libgenic/thermal.cpp as
genic/main.cpp:162-187 and 215-228 use them), written from the procedure and from the C++ standard's definition of ranlux48, for the
tests of shq_thermal_*.

ranlux48 = discard_block<subtract_with_carry<48, 5, 12>, 389, 11>:
  seed(v)  the LCG x <- 40014 x mod 2147483563 from v mod 2147483563 (1 if that is 0; v == 0 stands for 19780503); each of the 12 words
           takes two outputs, lo + (hi << 32) mod 2^48; carry = (word[11] == 0)
  step     y = word[k - 5] - word[k] - carry mod 2^48, carry = borrow, word[k] = y, k <- k + 1 mod 12
  block    11 steps are handed out, 378 are dropped
uniform_01<double> on it is one output times 2^-48: exact and below 1, so there is no redraw.
"""
import math

import numpy as np

NK = 2000
MAX_FERMI_DIRAC = 17.0
M48 = (1 << 48) - 1
LCG_A, LCG_M = 40014, 2147483563


def _seed_words(v):
    s = int(v) & 0xFFFFFFFF
    s = 19780503 if s == 0 else s
    s %= LCG_M
    if s == 0:
        s = 1
    x = []
    for _ in range(12):
        s = s * LCG_A % LCG_M
        lo = s
        s = s * LCG_A % LCG_M
        x.append((lo + (s << 32)) & M48)
    return x, int(x[11] == 0)


def ranlux48_stream(seed, m):
    """the first m outputs of ranlux48(seed) as Python ints: one serial stream"""
    x, c = _seed_words(seed)
    out = []
    k = 0
    while len(out) < m:
        for kept in (True, False):
            for _ in range(11 if kept else 378):
                y = x[k - 5] - x[k] - c
                c = 1 if y < 0 else 0
                y &= M48
                x[k] = y
                k = k + 1 if k < 11 else 0
                if kept:
                    out.append(y)
    return out[:m]


class Ranlux48:
    """one engine per seed, advanced together (numpy uint64 across the engines)"""

    def __init__(self, seeds):
        words = [_seed_words(v) for v in np.asarray(seeds).ravel()]
        self.x = np.array([w[0] for w in words], dtype=np.uint64)        # [S][12]
        self.c = np.array([w[1] for w in words], dtype=np.uint64)
        self.k = 0                                                        # the next word
        self.n = 0                                                        # outputs handed out of this block

    def _step(self):
        k = self.k
        y = self.x[:, (k - 5) % 12] - self.x[:, k] - self.c               # wraps mod 2^64; a borrow shows in bit 63
        self.c = y >> np.uint64(63)
        y = y & np.uint64(M48)
        self.x[:, k] = y
        self.k = (k + 1) % 12
        return y

    def next(self):
        if self.n == 11:
            for _ in range(378):
                self._step()
            self.n = 0
        self.n += 1
        return self._step()

    def outputs(self, m):
        return np.stack([self.next() for _ in range(m)], axis=1)          # [S][m]


def seed_table(Seed, Ngrid):
    """init_rng: Ngrid^2 outputs of ranlux48(Seed), i outer and j inner, truncated to 32 bits, at table[i + Ngrid * j]"""
    draws = np.array([d & 0xFFFFFFFF for d in ranlux48_stream(Seed, Ngrid * Ngrid)], dtype=np.uint32).reshape(Ngrid, Ngrid)   # [i][j]
    table = np.zeros(Ngrid * Ngrid, dtype=np.uint32)
    for i in range(Ngrid):
        for j in range(Ngrid):
            table[i + Ngrid * j] = draws[i, j]
    return table


def fd_kernel(x):
    return x * x / (np.exp(x) + 1)


def fd_tables(max_fd, min_fd=0.0):
    """init_thermalvel: (vel, cumprob, total_frac); 12-point Gauss-Legendre per knot interval"""
    max_fd = min(float(max_fd), MAX_FERMI_DIRAC)
    vel = min_fd + (max_fd - min_fd) * np.arange(NK) / (NK - 1.0)
    gx, gw = np.polynomial.legendre.leggauss(12)

    def panels(edges):
        mid, half = (edges[1:] + edges[:-1]) / 2, (edges[1:] - edges[:-1]) / 2
        return (fd_kernel(mid[:, None] + half[:, None] * gx[None, :]) * gw[None, :]).sum(axis=1) * half

    cum = np.concatenate([[0.0], np.cumsum(panels(vel))])
    total = panels(np.linspace(0.0, MAX_FERMI_DIRAC, 2001)).sum()
    return vel, cum / cum[-1], cum[-1] / total


def makima_slopes(x, y):
    """modified Akima: secants m, two ghost secants per side (m[-1] = 2 m[0] - m[1], ...), w1 = |m[i+1] - m[i]| + |m[i+1] + m[i]| / 2,
    w2 = |m[i-1] - m[i-2]| + |m[i-1] + m[i-2]| / 2, s[i] = (w1 m[i-1] + w2 m[i]) / (w1 + w2), 0 where both weights vanish"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    m = np.zeros(n + 3)                                                   # m[i + 2] is the secant of [x[i], x[i+1]], i = -2 .. n
    m[2:n + 1] = (y[1:] - y[:-1]) / (x[1:] - x[:-1])
    m[1] = 2 * m[2] - m[3]
    m[0] = 2 * m[1] - m[2]
    m[n + 1] = 2 * m[n] - m[n - 1]
    m[n + 2] = 2 * m[n + 1] - m[n]
    i = np.arange(n) + 2
    w1 = np.abs(m[i + 1] - m[i]) + np.abs(m[i + 1] + m[i]) / 2
    w2 = np.abs(m[i - 1] - m[i - 2]) + np.abs(m[i - 1] + m[i - 2]) / 2
    w = w1 + w2
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(w > 0, (w1 * m[i - 1] + w2 * m[i]) / w, 0.0)


def find_bin(x, p):
    """the last knot with x[i] <= p, at most len(x) - 2"""
    return np.clip(np.searchsorted(x, p, side="right") - 1, 0, len(x) - 2)


def hermite(x, y, s, p):
    """(F(p), bin): the cubic Hermite through the knots with slopes s, every operation in this order"""
    p = np.asarray(p, dtype=np.float64)
    i = find_bin(x, p)
    dx = x[i + 1] - x[i]
    d = p - x[i]
    t = d / dx
    omt = 1 - t
    a = y[i] * (1 + 2 * t) + s[i] * d
    b = y[i + 1] * (3 - 2 * t) + (dx * s[i + 1]) * (t - 1)
    return (omt * omt) * a + (t * t) * b, i


def add_thermal_speeds(v_amp, cumprob, fdvel, slopes, raw3):
    """the three draws raw3 [.., 3] (engine outputs) of each particle -> (dvel [.., 3], speed, bin); libm through Python's math module"""
    u = np.asarray(raw3, dtype=np.uint64).astype(np.float64) * 2.0 ** -48
    F, ibin = hermite(cumprob, fdvel, slopes, u[..., 0])
    v = v_amp * F
    phi = (2 * math.pi) * u[..., 1]
    theta = np.vectorize(math.acos, otypes=[np.float64])(2 * u[..., 2] - 1)
    sin, cos = np.vectorize(math.sin, otypes=[np.float64]), np.vectorize(math.cos, otypes=[np.float64])
    vs = v * sin(theta)
    return np.stack([vs * cos(phi), vs * sin(phi), v * cos(theta)], axis=-1), v, ibin


def thermal_speeds(vel, Ngrid, v_amp, seedtable, cumprob, fdvel, x0=0, nx=None, y0=0, ny=None):
    """the particle loop of genic/main.cpp:176-184 over the sub-block's particles: local index i is x = i / (ny Ngrid) + x0,
    y = (i mod (ny Ngrid)) / Ngrid + y0, z = i mod Ngrid; id = x Ngrid^2 + y Ngrid + z + 1; the engine is reseeded with
    seedtable[id / Ngrid] where z == 0.  Returns dict(Vel float32, dvel, speed, bin)."""
    nx = Ngrid - x0 if nx is None else nx
    ny = Ngrid - y0 if ny is None else ny
    vel = np.asarray(vel, dtype=np.float32)
    n = nx * ny * Ngrid
    assert vel.shape == (n, 3)
    first = np.arange(0, n, Ngrid)
    ids = (first // (ny * Ngrid) + x0) * Ngrid * Ngrid + ((first % (ny * Ngrid)) // Ngrid + y0) * Ngrid + 0 + 1
    eng = Ranlux48(np.asarray(seedtable)[ids // Ngrid])
    raw = eng.outputs(3 * Ngrid).reshape(nx * ny * Ngrid, 3)              # column-major over z: exactly the particle order
    dvel, speed, ibin = add_thermal_speeds(v_amp, cumprob, fdvel, makima_slopes(cumprob, fdvel), raw)
    out = (vel.astype(np.float64) + dvel).astype(np.float32)
    return dict(Vel=out, dvel=dvel, speed=speed, bin=ibin)
