"""A numpy restatement of the initial-condition displacements (displacement_fields, libgenic/zeldovich.cpp:150-264) for one rank: the
Gaussian fill (gaussian_fill, zeldovich.cpp:362-383; pmic_fill_gaussian_gadget with SETSEED / SAMPLE, libgenic/pmesh.h:18-178), the
transfer functions (zeldovich.cpp:277-334) on pm_apply_transfer_function's mode enumeration (petapm.cpp:1258-1298), the CIC readout
(pm_iterate_one, petapm.cpp:1133-1183) and the final particle loop.

pmesh.h needs boost, which the reference's own tests do not exercise for this path: there is no reference output to pin this against.
It is a line-by-line restatement.  What pins it independently: the engine (the C++ standard's 10000th output of mt19937(5489)), the
variate (draw / 2^32, the reading of boost's uniform_real_distribution that orc.boost_mt19937_uniform uses), and the structure the
reference relies on (tests/test_zeldovich_cpu.py).

The fill here is the literal procedure: TWO generators per column (this_rng, lower_rng), one SAMPLE each per k in the order use_conj
decides, the ampl == 0 redraw.  init_genrand and the twist are vectorised across generators; nothing else is rearranged."""
import numpy as np

UPPER, LOWER, MAG = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)


def init_genrand(seeds):
    """mt19937's seeding for an array of seeds: [n][624] uint32"""
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    mt = np.zeros((len(seeds), 624), dtype=np.uint64)
    mt[:, 0] = seeds
    for i in range(1, 624):
        p = mt[:, i - 1]
        mt[:, i] = (np.uint64(1812433253) * (p ^ (p >> np.uint64(30))) + np.uint64(i)) & np.uint64(0xFFFFFFFF)
    return mt.astype(np.uint32)


def twist(mt):
    """genrand's block regeneration of all 624 words, in place, every generator at once: word i from i, i + 1 and i + 397"""
    def seg(lo, hi, src):
        y = (mt[:, lo:hi] & UPPER) | (mt[:, lo + 1:hi + 1] & LOWER)
        mt[:, lo:hi] = mt[:, src:src + hi - lo] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), MAG, np.uint32(0))
    seg(0, 227, 397)
    seg(227, 454, 0)
    seg(454, 623, 227)
    y = (mt[:, 623] & UPPER) | (mt[:, 0] & LOWER)
    mt[:, 623] = mt[:, 396] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), MAG, np.uint32(0))


def temper(y):
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xEFC60000))
    return y ^ (y >> np.uint32(18))


def raw_outputs(states, m):
    """the first m 32-bit outputs of generators whose 624 words are `states` before their first twist: [n][m] uint32"""
    mt = np.array(states, dtype=np.uint32, copy=True).reshape(-1, 624)
    out = []
    for _ in range((m + 623) // 624):
        twist(mt)
        out.append(temper(mt))
    return np.concatenate(out, axis=1)[:, :m]


class Generators:
    """n independent mt19937 behind boost's uniform_real_distribution<double>(0, 1): dist(rng) = draw / 2^32, each generator with its own
    cursor (a redraw shifts that generator's stream from there on)"""

    def __init__(self, states, ndraws):
        self.raw = raw_outputs(states, ndraws)
        self.cur = np.zeros(self.raw.shape[0], dtype=np.int64)
        self.rows = np.arange(self.raw.shape[0])

    def dist(self, mask=None):
        rows = self.rows if mask is None else self.rows[mask]
        if (self.cur[rows] >= self.raw.shape[1]).any():
            raise RuntimeError("Generators: more draws than were prepared")
        u = self.raw[rows, self.cur[rows]].astype(np.float64) / 4294967296.0
        self.cur[rows] += 1
        return u

    def sample(self):
        """SAMPLE (pmesh.h:55-62): phase = dist * 2 * M_PI; do ampl = dist while(ampl == 0)"""
        phase = self.dist() * 2 * np.pi
        ampl = self.dist()
        while True:
            z = ampl == 0
            if not z.any():
                return ampl, phase
            ampl[z] = self.dist(z)


def sample_pairs(states, m):
    """the first m // 2 SAMPLEs of each generator as (phase, ampl before the log): [n][m // 2][2]"""
    g = Generators(states, 2 * m + 64)
    out = np.zeros((g.raw.shape[0], m // 2, 2))
    for q in range(m // 2):
        ampl, phase = g.sample()
        out[:, q, 0], out[:, q, 1] = phase, ampl
    return out


def seed_table(N, Seed):
    """SETSEED and the eight loops of pmesh.h:18-41, 81-90 on one rank; returns table[d1][d2] as [N][N] uint32 arrays"""
    calls = []
    for i in range(N // 2):
        calls += [(i, j) for j in range(i)]
        calls += [(j, i) for j in range(i + 1)]
        calls += [(N - 1 - i, j) for j in range(i)]
        calls += [(N - 1 - j, i) for j in range(i + 1)]
        calls += [(i, N - 1 - j) for j in range(i)]
        calls += [(j, N - 1 - i) for j in range(i + 1)]
        calls += [(N - 1 - i, N - 1 - j) for j in range(i)]
        calls += [(N - 1 - j, N - 1 - i) for j in range(i + 1)]
    u = raw_outputs(init_genrand([Seed & 0xFFFFFFFF]), max(len(calls), 1))[0].astype(np.float64) / 4294967296.0
    seeds = (float(0x7FFFFFFF) * u).astype(np.uint32)       # static_cast<unsigned int>(0x7fffffff * dist(rng))
    table = [[np.zeros((N, N), dtype=np.uint32) for _ in range(2)] for _ in range(2)]
    for (i, j), s in zip(calls, seeds):
        ii, jj = (i, (N - i) % N), (j, (N - j) % N)
        for d1 in range(2):
            for d2 in range(2):
                table[d1][d2][ii[d1], jj[d2]] = s
    return table


def fill_gaussian(N, Seed, UnitaryAmplitude=0, InvertPhase=0, columns=None, table=None):
    """pmic_fill_gaussian_gadget (pmesh.h:64-178) for the columns c = i * N + j of `columns` (default: all): delta_k[i][j][k], zero
    elsewhere.  gaussian_fill's axis permutation makes pmesh's (i, j, k) petapm's (x, y, z'): the result is the dense [x][y][z'] half
    spectrum; reference_layout() gives petapm's [y][z'][x]."""
    table = seed_table(N, Seed) if table is None else table
    cols = np.arange(N * N) if columns is None else np.asarray(columns, dtype=np.int64)
    i, j = cols // N, cols % N
    ci, cj = (N - i) % N, (N - j) % N
    d = ((ci == i) & (cj < j)) | ((ci < i) & (cj != j)) | ((ci < i) & (cj == j))
    t11, t00 = table[1][1][i, j], table[0][0][i, j]
    seed_conj = np.where(d, t11, t00)                         # GETSEED(i, j, d1, d2)
    seed_this = t00
    ndraws = 2 * (N // 2 + 1) + 64
    lower, this = Generators(init_genrand(seed_conj), ndraws), Generators(init_genrand(seed_this), ndraws)
    out = np.zeros((N, N, N // 2 + 1), dtype=np.complex128)
    for k in range(N // 2 + 1):
        use_conj = d & (k == 0 or k == N // 2)
        # use_conj: SAMPLE(this), then SAMPLE(lower); otherwise SAMPLE(lower), then SAMPLE(this): the second call's values stay
        a_t, p_t = this.sample()
        a_l, p_l = lower.sample()
        ampl, phase = np.where(use_conj, a_l, a_t), np.where(use_conj, p_l, p_t)
        ampl = np.sqrt(-np.log(ampl))
        if UnitaryAmplitude:
            ampl = np.ones_like(ampl)
        if InvertPhase:
            phase = phase + np.pi
        re, im = ampl * np.cos(phase), ampl * np.sin(phase)
        im = np.where(use_conj, im * -1, im)
        selfc = ((N - i) % N == i) & ((N - j) % N == j) & ((N - k) % N == k)
        im = np.where(selfc, 0.0, im)
        zero = (i == 0) & (j == 0) & (k == 0)
        re, im = np.where(zero, 0.0, re), np.where(zero, 0.0, im)
        out[i, j, k] = re + 1j * im
    return out


def reference_layout(dense):
    """[x][y][z'] -> petapm's Fourier layout [y][z'][x]"""
    return np.ascontiguousarray(dense.transpose(1, 2, 0))


def tabulate_k2(fn, N, BoxSize):
    """fn(kmag) at kmag = sqrt(k2) * 2 * M_PI / BoxSize for k2 = 0 .. 3 (N/2)^2 (entry 0 is never read: 0)"""
    k2 = np.arange(3 * (N // 2) ** 2 + 1)
    t = np.zeros(len(k2))
    t[1:] = fn(np.sqrt(k2[1:]) * 2 * np.pi / BoxSize)
    return t


def transfer_meshes(spec_yzx, N, BoxSize, delta, growth=None):
    """pm_apply_transfer_function on [y][z'][x] with density_transfer / disp_transfer, then the unscaled c2r: the real meshes [x][y][z] of
    Density, DispX/Y/Z and, with a growth table, VelX/Y/Z"""
    k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N)
    ky, kz, kx = np.meshgrid(k1, k1[: N // 2 + 1], k1, indexing="ij")    # pos[] = (y, z, x) -> kpos handed on as (kx, ky, kz)
    k2 = kx.astype(np.int64) ** 2 + ky.astype(np.int64) ** 2 + kz.astype(np.int64) ** 2
    nz = k2 > 0
    k2s = np.where(nz, k2, 1)
    meshes = []

    def c2r(e):
        return np.fft.irfftn(e.transpose(2, 0, 1), s=(N, N, N), axes=(0, 1, 2)) * float(N) ** 3

    r2 = 1.0 / N
    r2 *= r2
    fac = np.exp(-k2s * r2)
    fac = fac * (delta[k2s] / np.sqrt(BoxSize * BoxSize * BoxSize))
    meshes.append(c2r(np.where(nz, spec_yzx * fac, spec_yzx)))
    for tab in ([delta] if growth is None else [delta, growth]):
        for kaxis in (kx, ky, kz):
            fac = 1.0 / (2 * np.pi) / np.sqrt(BoxSize) * kaxis / k2s
            fac = fac * tab[k2s]
            e = (-spec_yzx.imag * fac) + 1j * (spec_yzx.real * fac)
            meshes.append(c2r(np.where(nz, e, spec_yzx)))
    return meshes


def cic_readout(mesh, pos, N, BoxSize):
    """pm_iterate_one's gather: the 8 connections in their order, weight = the product over k of Res or 1 - Res"""
    cellsize = BoxSize / N
    tmp = pos / cellsize
    cell = np.floor(tmp)
    res = tmp - cell
    cell = cell.astype(np.int64)
    acc = np.zeros(len(pos))
    for connection in range(8):
        weight = np.ones(len(pos))
        idx = []
        for k in range(3):
            off = (connection >> k) & 1
            idx.append((cell[:, k] + off) % N)
            weight = weight * (res[:, k] if off else (1 - res[:, k]))
        acc = acc + weight * mesh[idx[0], idx[1], idx[2]]
    return acc


def periodic_wrap(x, L):
    x = np.array(x, dtype=np.float64, copy=True)
    while (x >= L).any():
        x[x >= L] -= L
    while (x < 0).any():
        x[x < 0] += L
    return x


def displacement_fields(N, BoxSize, Seed, UnitaryAmplitude, InvertPhase, vel_prefac, ScaleDepVelocity, delta, growth, pos, spec=None):
    """displacement_fields for one rank; returns dict(Pos, Vel, Density, Disp, maxdisp, maxvel)"""
    if spec is None:
        spec = reference_layout(fill_gaussian(N, Seed, UnitaryAmplitude, InvertPhase))
    meshes = transfer_meshes(spec, N, BoxSize, delta, growth if ScaleDepVelocity else None)
    density = cic_readout(meshes[0], pos, N, BoxSize)
    disp = np.stack([cic_readout(meshes[1 + k], pos, N, BoxSize) for k in range(3)], axis=1)
    vel = np.stack([cic_readout(meshes[4 + k], pos, N, BoxSize) for k in range(3)], axis=1) if ScaleDepVelocity else disp.copy()
    maxdisp = max(0.0, disp.max()) if len(pos) else 0.0
    newpos = pos + disp
    vel = vel * vel_prefac
    absv = np.zeros(len(pos))
    for k in range(3):
        absv = absv + vel[:, k] * vel[:, k]
    maxvel = max(0.0, absv.max()) if len(pos) else 0.0
    return dict(Pos=periodic_wrap(newpos, BoxSize), Vel=vel, Density=density, Disp=disp, maxdisp=maxdisp, maxvel=maxvel, meshes=meshes)


def idgen_positions(Ngrid, BoxSize, shift=0.0):
    """setup_grid with idgen_create_pos_from_index on one rank (zeldovich.cpp:77-104): index = (x * Ngrid + y) * Ngrid + z"""
    idx = np.arange(Ngrid**3)
    x, y, z = idx // (Ngrid * Ngrid), (idx % (Ngrid * Ngrid)) // Ngrid, idx % Ngrid
    pos = np.stack([x * BoxSize / Ngrid, y * BoxSize / Ngrid, z * BoxSize / Ngrid], axis=1)
    return pos + shift
