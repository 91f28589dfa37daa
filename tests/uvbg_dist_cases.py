"""Shared inputs of the sharded excursion-set reionisation tests (test_dist_uvbg_cpu.py, test_gpu_dist_uvbg.py): the particle recipe of
test_gpu_uvbg with two star clusters moved onto slab boundaries, the reference (uvbg_restated.calculate_uvbg on the undivided set,
computed once per case), the comparison rules of test_parity_with_the_restatement, what a case has to cover, a numpy stand-in for
DistUVBG's ops, and the per-rank run."""
import functools
import math

import numpy as np
import torch

import uvbg_restated as ur
from test_gpu_uvbg import BOX, COSMO, _params, _particles, _structs, _ulps

# (UVBGdim, ranks, ReionFilterType, RtoMFilterType, ReionUseParticleSFR); 36 has no bespoke transform (torch.fft route)
CASES = [(32, 2, 0, 0, 0), (48, 2, 2, 0, 1), (48, 3, 0, 1, 1), (64, 4, 1, 0, 0), (36, 2, 2, 0, 1)]
SEED = 5
NEAR_CAP = 1e-3          # cells left out as `near` the threshold: at most 0.1 % of the mesh


@functools.lru_cache(maxsize=None)
def particles(N, size, seed=SEED, stars=True):
    """_particles(N, seed) with the strongest star cluster centred on the cut between rank 0 and rank 1, x = (N / size) cell, and the
    second strongest on the box wrap, x = 0: the recipe's own draws with those two centres' x replaced."""
    pos, types, mass, fesc, sfr, lj, zr = _particles(N, seed, stars)
    if stars:
        rng = np.random.default_rng(seed)          # the recipe's stream again, for the centres it drew
        rng.normal(0, 1, (N ** 3, 3))
        rng.normal(0, 1, (N ** 3, 3))
        first = 2 * N ** 3
        pos = pos.copy()
        for k in range(6):
            c = rng.uniform(0, BOX, 3)
            m = 12 + 6 * k
            rng.normal(0, 1, (m, 3))
            target = {5: (N // size) * (BOX / N), 4: 0.0}.get(k)
            if target is not None:
                assert (types[first:first + m] == 4).all()
                pos[first:first + m, 0] = np.mod(pos[first:first + m, 0] - c[0] + target, BOX)
            first += m
        assert first == len(pos)
    for a in (pos, types, mass, fesc, sfr, lj, zr):
        a.setflags(write=False)
    return pos, types, mass, fesc, sfr, lj, zr


@functools.lru_cache(maxsize=None)
def reference(N, size, ftype, rtom, use_sfr, seed=SEED, stars=True, **kw):
    pos, types, mass, fesc, sfr, lj, zr = particles(N, size, seed, stars)
    return ur.calculate_uvbg(_params(N, ftype, rtom, use_sfr, **kw), COSMO, pos, mass, types, fesc, sfr, lj, zr)


def assert_coverage(ref, N, size, seed=SEED):
    """what a case must exercise, on the reference: ionised cells either side of the cut and at the wrap, and gas whose zreion the
    step sets in the last plane of rank 0's slab and in the last plane of the box - right only with the neighbour's J21 plane"""
    pos, types, _, _, _, _, zr = particles(N, size, seed)
    cut = N // size
    ion = ref["xHI"] == 0
    assert ion[cut - 1].any() and ion[cut].any(), (int(ion[cut - 1].sum()), int(ion[cut].sum()))
    assert ion[N - 1].any() or ion[0].any()
    plane = np.floor(pos[:, 0] / (BOX / N)).astype(np.int64) % N
    newly = (types == 0) & (ref["zreion"] != zr)
    assert (newly & (plane == cut - 1)).any() and (newly & (plane == N - 1)).any()
    assert int(ref["near"].sum()) <= NEAR_CAP * N ** 3


def compare(got, ref, N, size, seed=SEED, stars=True):
    """the rules of test_parity_with_the_restatement plus the cap on `near`; got: J21, xHI [N]^3, vol, mass, nradii, fesc,
    local_J21, zreion in the global particle order"""
    _, types, _, _, _, lj, zr = particles(N, size, seed, stars)
    near = ref["near"]
    assert int(near.sum()) <= NEAR_CAP * N ** 3
    assert got["nradii"] == ref["nradii"]
    ion = ref["xHI"] == 0
    flip = (ion != (got["xHI"] == 0)) & ~near
    assert not flip.any(), np.argwhere(flip)[:10]
    ok = ~near
    floor = 1e-12 * float(ref["J21"].max())
    jbad = (_ulps(got["J21"], ref["J21"]) > 1) & (np.abs(got["J21"].astype(np.float64) - ref["J21"]) > floor)
    assert not jbad[ok].any(), (np.argwhere(jbad & ok)[:10], got["J21"][jbad & ok][:10], ref["J21"][jbad & ok][:10])
    assert _ulps(got["xHI"], ref["xHI"])[ok].max() <= 1
    assert abs(got["vol"] - ref["vol"]) <= 1e-12 and abs(got["mass"] - ref["mass"]) <= 1e-12, (got["vol"], ref["vol"], got["mass"], ref["mass"])
    assert np.allclose(got["fesc"], ref["fesc"], rtol=4e-16, atol=0)
    pnear = near.reshape(-1)[ref["cells"]].any(axis=1)
    gas = (types == 0) & ~pnear
    lbad = (_ulps(got["local_J21"], ref["local_J21"]) > 1) & (np.abs(got["local_J21"] - ref["local_J21"]) > floor)
    assert not lbad[gas].any()
    zok = ~pnear & (ref["local_J21"] > floor)
    zok |= ~pnear & (types != 0)
    assert np.array_equal(got["zreion"][zok], ref["zreion"][zok])
    assert np.array_equal(got["zreion"][types != 0], zr[types != 0])
    assert np.array_equal(got["local_J21"][types != 0], lj[types != 0])       # only gas is written


class RestatedUvbgOps:
    """DistUVBG's ops in numpy, from the restatement's pieces (init_particle_uvbg, _cic, filter_table, the cell loop of
    calculate_uvbg) on a rank's planes; the deposit is the library's fixed point, so that ghost planes add exactly."""
    device = torch.device("cpu")

    def pitch(self):
        return 0

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype)

    def fesc(self, p, cosmo, posm, types, fesc, sfr):
        t, m = types.numpy(), posm[:, 3].numpy()
        use_sfr = bool(p.ReionUseParticleSFR)
        neg = False
        try:
            fesc.copy_(torch.from_numpy(ur.init_particle_uvbg(t, fesc.numpy(), use_sfr, p.EscapeFractionNorm, p.EscapeFractionScaling,
                                                              cosmo.UnitMass_in_g, cosmo.HubbleParam)))
        except ValueError:
            neg = True
        f = fesc.numpy()
        return [np.abs(m).sum(), np.abs(m * f)[t == 4].sum(), np.abs(sfr.numpy() * f)[(t == 0) & use_sfr].sum()], neg

    def tables(self, p, radii):
        self.tabs = [ur.filter_table(p.ReionFilterType, p.UVBGdim, p.BoxSize, R) for R in radii[:-1]] + [None]

    def _local_cells(self, posm, N, L, plane0, nalloc):
        idx, wts = ur._cic(posm[:, 0:3].numpy(), N, L / N)
        loc = []
        for lin in idx:
            ix = (lin // (N * N) - plane0) % N
            assert (ix < nalloc).all(), "a particle outside this rank's slab"
            loc.append(ix * N * N + lin % (N * N))
        return loc, wts

    def deposit(self, p, posm, types, fesc, sfr, exps, plane0, nxl, nalloc):
        N, t = p.UVBGdim, types.numpy()
        loc, wts = self._local_cells(posm, N, p.BoxSize, plane0, nalloc)
        m, f = posm[:, 3].numpy(), fesc.numpy()
        fields = [(m, np.ones(len(t), bool)), (m * f, t == 4)] + ([(sfr.numpy() * f, t == 0)] if p.ReionUseParticleSFR else [])
        out = []
        for (value, sel), e in zip(fields, exps):
            mesh = np.zeros(nalloc * N * N, dtype=np.int64)
            for lin, w in zip(loc, wts):
                np.add.at(mesh, lin[sel], np.rint((w * value)[sel] * math.ldexp(1.0, 61 - e)).astype(np.int64))
            out.append(torch.from_numpy(mesh.reshape(nalloc, N, N)))
        return out

    def to_real(self, mesh_i, exp):
        return mesh_i.to(torch.float64) * math.ldexp(1.0, exp - 61)

    def filter(self, spec_t, y0, nyl, r):
        N = spec_t.shape[0]
        k1 = np.fft.fftfreq(N, 1.0 / N).astype(np.int64)
        k2 = k1[:, None, None] ** 2 + k1[None, y0:y0 + nyl, None] ** 2 + np.arange(N // 2 + 1)[None, None, :] ** 2
        T = np.ones(k2.shape) if self.tabs[r] is None else self.tabs[r][k2]
        return torch.from_numpy(spec_t.numpy() / (N * N * N) * T)

    def cells(self, p, cp, R, last, meshes, zp, nxl, J21, xHI):
        """reion_loop_pm as uvbg_restated.calculate_uvbg states it, on this rank's planes"""
        N, L = p.UVBGdim, p.BoxSize
        real = [m.numpy()[:nxl, :, :N] for m in meshes]
        J, x = J21.numpy(), xHI.numpy()
        cell = L / N
        redshift = 1.0 / cp.Time - 1.
        eff = 1.0 / (cp.OmegaBaryon / cp.Omega0) * p.ReionNionPhotPerBary / (1.0 - 0.75 * (1.0 - ur.HYDROGEN_MASSFRAC))
        pixel_volume = cell * cell * cell
        dconv = float(N * N * N) / (cp.RhoCrit * cp.Omega0 * L * L * L)
        hubble_time = 1 / (cp.hubble * cp.HubbleParam)
        mass_real, star_real = np.maximum(real[0], 0.0), np.maximum(real[1], 0.0)
        if p.RtoMFilterType == 0:
            RtoM = (4.0 / 3.0) * math.pi * ur._libm.pow(R, 3) * (cp.Omega0 * cp.RhoCrit)
        else:
            RtoM = ur._libm.pow(2 * math.pi, 1.5) * cp.Omega0 * cp.RhoCrit * ur._libm.pow(R, 3)
        Jc = ((1.0 + redshift) * (1.0 + redshift) / (4.0 * math.pi) * p.AlphaUV * ur.PLANCK * 1e21 * R * cp.UnitLength_in_cm
              * p.ReionNionPhotPerBary / ur.PROTONMASS * cp.UnitMass_in_g / ur._libm.pow(cp.UnitLength_in_cm, 3) / cp.UnitTime_in_s)
        with np.errstate(divide="ignore", invalid="ignore"):
            f_coll = star_real / (RtoM * (mass_real * dconv)) * (4.0 / 3.0) * math.pi * R * R * R / pixel_volume
        if p.ReionUseParticleSFR:
            sfr_density = np.maximum(real[2], 0.0) / pixel_volume / (cp.UnitMass_in_g / ur.SOLAR_MASS) * (cp.UnitTime_in_s / ur.SEC_PER_YEAR)
        else:
            sfr_density = star_real / (p.ReionSFRTimescale * hubble_time) / pixel_volume
        J_aux = (sfr_density * Jc).astype(np.float32)
        ion = f_coll > 1.0 / eff
        first = ion & (x > ur.FLOAT_REL_TOL)
        J[first] = J_aux[first]
        x[ion] = 0.0
        if not last:
            return None
        part = ~ion & (x > ur.FLOAT_REL_TOL)
        x[part] = (1.0 - f_coll[part] * eff).astype(np.float32)
        d = dconv * mass_real
        return [float(x.astype(np.float64).sum()), float((x.astype(np.float64) * d).sum()), float(d.sum())]

    def readout(self, p, cp, posm, types, J21ext, plane0, nxl, local_J21, zreion):
        loc, _ = self._local_cells(posm, p.UVBGdim, p.BoxSize, plane0, J21ext.shape[0])
        gas = types.numpy() == 0
        lj, zr = local_J21.numpy(), zreion.numpy()
        lj[gas] = 0.0
        Jf = J21ext.numpy().reshape(-1).astype(np.float64)
        for lin in loc:
            v = Jf[lin]
            up = gas & (v > lj)
            lj[up] = v[up]
            zr[up & (zr == -1)] = 1 / cp.Time - 1


def deal(n, size, how):
    """which rank holds which particle: at random (not by slab, so the routing and the way back are exercised); how = the seed"""
    return np.random.default_rng(how).integers(0, size, n)


def run_rank(comm, ops, case, how=1, seed=SEED, stars=True, bounds=None, holder=None, **kw):
    """one rank's call on its share of the case's particles; holder (n ranks) overrides the random deal"""
    from shenqi_amd import dist as sd
    N, size, ftype, rtom, use_sfr = case
    pos, types, mass, fesc, sfr, lj, zr = particles(N, size, seed, stars)
    who = deal(len(pos), comm.size, how) if holder is None else holder
    idx = np.flatnonzero(who == comm.rank)
    p, cp = _structs(_params(N, ftype, rtom, use_sfr, **kw), COSMO)
    drv = sd.DistUVBG(comm, N, BOX, ops, bounds)
    arrs = [a[idx].copy() for a in (fesc, sfr, lj, zr)]
    before = [a.copy() for a in arrs]
    try:
        vol, mw, nr = drv.calculate(p, cp, pos[idx], mass[idx], types[idx], *arrs)
    except ValueError as e:
        return dict(error=str(e), untouched=all(np.array_equal(a, b) for a, b in zip(arrs, before)), idx=idx)
    return dict(idx=idx, fesc=arrs[0], local_J21=arrs[2], zreion=arrs[3], vol=vol, mass=mw, nradii=nr, plane0=drv.d.plane0,
                J21=drv.J21.cpu().numpy().copy(), xHI=drv.xHI.cpu().numpy().copy(), rows_sent=drv.rows_sent, nalltoall=drv.nalltoall)


def assemble(results, N):
    """the ranks' results as one: the grids by plane, the particle arrays in the global order"""
    n = sum(len(r["idx"]) for r in results)
    got = dict(J21=np.empty((N, N, N), np.float32), xHI=np.empty((N, N, N), np.float32), nradii=results[0]["nradii"], vol=results[0]["vol"],
               mass=results[0]["mass"])
    for k in ("fesc", "local_J21", "zreion"):
        got[k] = np.empty(n)
    for r in results:
        assert (r["vol"], r["mass"], r["nradii"]) == (got["vol"], got["mass"], got["nradii"])       # every rank returns the same
        w = r["J21"].shape[0]
        got["J21"][r["plane0"]:r["plane0"] + w], got["xHI"][r["plane0"]:r["plane0"] + w] = r["J21"], r["xHI"]
        for k in ("fesc", "local_J21", "zreion"):
            got[k][r["idx"]] = r[k]
    return got
