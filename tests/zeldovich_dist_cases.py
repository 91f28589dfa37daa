"""Shared pieces of the sharded Zel'dovich tests (test_dist_zeldovich_cpu.py, test_gpu_dist_zeldovich.py): the cases, the particles (a
lattice on cell edges and slab cuts plus random points), the reference (zeldovich_restated.displacement_fields on the undivided set,
computed once per case), a numpy stand-in for DistZeldovich's ops, and the per-rank run with its assembly."""
import functools

import numpy as np
import torch

import zeldovich_restated as zr
from test_gpu_zeldovich import BAR, BOX, _compare, _tables  # noqa: F401

# (Nmesh, ranks, ScaleDepVelocity); 18 has no bespoke transform (torch.fft route)
CASES = [(16, 2, 0), (24, 3, 1), (16, 4, 1), (18, 2, 1)]
SEED = 181170
VEL_PREFAC = 37.5
FIELDS = ("Pos", "Vel", "Density", "Disp")


@functools.lru_cache(maxsize=None)
def particles(N):
    """the Ngrid = N / 2 lattice shifted by half a lattice cell - one mesh cell, so every lattice point sits on a cell edge (residual 0)
    and a plane of them on every slab cut - and 500 uniform random points"""
    Ngrid = N // 2
    pos = np.concatenate([zr.idgen_positions(Ngrid, BOX, 0.5 * BOX / Ngrid), np.random.default_rng(N).uniform(0, BOX, (500, 3))])
    assert pos.min() >= 0 and pos.max() < BOX
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def reference(N, scaledep, other=False, seed=SEED):
    delta, growth = _tables(N, other)
    ref = zr.displacement_fields(N, BOX, seed, 0, 0, VEL_PREFAC, scaledep, delta, growth, particles(N))
    ref.pop("meshes")
    return ref


def deal(n, size, how):
    """which rank holds which particle: 1 round-robin, 2 blocks in reversed rank order (neither is by slab, so the routing and the
    way back are exercised)"""
    return np.arange(n) % size if how == 1 else size - 1 - np.arange(n) * size // n


class RestatedZeldovichOps:
    """DistZeldovich's ops in numpy from the restatement's pieces: the fill is zr.fill_gaussian of the slab's columns, the transfer
    has transfer_meshes' operation order, the gather is cic_readout on the rank's window; the transforms are the driver's torch.fft."""
    device = torch.device("cpu")

    def pitch(self, N):
        return 0

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype)

    def fill(self, N, Seed, unitary, invert, y0, nyl):
        cols = (np.arange(N)[:, None] * N + np.arange(y0, y0 + nyl)[None, :]).reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(zr.fill_gaussian(N, Seed, unitary, invert, columns=cols)[:, y0:y0 + nyl]))

    def tables(self, N, L, delta, growth):
        self.tabs = (delta, growth)

    def transfer(self, N, L, spec, y0, nyl, field):
        delta, growth = self.tabs
        s = spec.numpy()
        k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N).astype(np.int64)
        kx, ky, kz = np.meshgrid(k1, k1[y0:y0 + nyl], k1[:N // 2 + 1], indexing="ij")
        k2 = kx ** 2 + ky ** 2 + kz ** 2
        nz = k2 > 0
        k2s = np.where(nz, k2, 1)
        if field == 0:
            r2 = 1.0 / N
            r2 *= r2
            fac = np.exp(-k2s * r2)
            fac = fac * (delta[k2s] / np.sqrt(L * L * L))
            e = s * fac
        else:
            fac = 1.0 / (2 * np.pi) / np.sqrt(L) * (kx, ky, kz)[(field - 1) % 3] / k2s
            fac = fac * (delta if field < 4 else growth)[k2s]
            e = (-s.imag * fac) + 1j * (s.real * fac)
        return torch.from_numpy(np.where(nz, e, s))

    def gather(self, N, L, pos, window, plane0, nxl, out):
        w, p = window.numpy(), pos.numpy()
        tmp = p / (L / N)
        cell = np.floor(tmp)
        res = tmp - cell
        cell = cell.astype(np.int64)
        acc = np.zeros(len(p))
        for connection in range(8):
            weight = np.ones(len(p))
            idx = []
            for k in range(3):
                off = (connection >> k) & 1
                idx.append((cell[:, k] + off) % N)
                weight = weight * (res[:, k] if off else (1 - res[:, k]))
            ix = (idx[0] - plane0) % N
            assert (ix < w.shape[0]).all(), "a particle outside this rank's slab"
            acc = acc + weight * w[ix, idx[1], idx[2]]
        out.copy_(torch.from_numpy(acc))

    def finalize(self, pos, fld, scaledep, vel_prefac, L):
        p, f = pos.numpy(), fld.numpy()
        disp = np.ascontiguousarray(f[1:4].T)
        vel = (np.ascontiguousarray(f[4:7].T) if scaledep else disp.copy()) * vel_prefac
        absv = np.zeros(len(p))
        for k in range(3):
            absv = absv + vel[:, k] * vel[:, k]
        mx = [max(0.0, disp.max()) if len(p) else 0.0, max(0.0, absv.max()) if len(p) else 0.0]
        return torch.from_numpy(zr.periodic_wrap(p + disp, L)), torch.from_numpy(vel), torch.from_numpy(disp), mx


def params(N, scaledep, seed=SEED, box=BOX, unitary=0, invert=0):
    from shenqi_amd import capi
    return capi.ZeldovichParams(N, seed, unitary, invert, scaledep, 0, box, VEL_PREFAC)


def run_rank(comm, ops, case, how=1, holder=None, pos=None, box=BOX, tables=None, drv=None, other=False, seed=SEED):
    """one rank's call on its share of the case's particles; holder (n ranks) overrides the deal, pos / box / tables the inputs"""
    from shenqi_amd import dist as sd
    N, size, scaledep = case
    pos = particles(N) if pos is None else pos
    who = deal(len(pos), comm.size, how) if holder is None else holder
    idx = np.flatnonzero(who == comm.rank)
    delta, growth = _tables(N, other) if tables is None else tables
    try:
        drv = sd.DistZeldovich(comm, N, box, ops) if drv is None else drv
    except ValueError as e:
        return dict(error=str(e), constructor=True)
    try:
        got = drv.displacements(params(N, scaledep, seed, box), delta, growth if scaledep else None, pos[idx])
    except ValueError as e:
        return dict(error=str(e), nalltoall=drv.nalltoall, idx=idx)
    got.update(idx=idx, rows_sent=drv.rows_sent, nalltoall=drv.nalltoall, filled=drv.filled, plane0=drv.d.plane0)
    return got


def assemble(results):
    """the ranks' results as one, in the global particle order; the two maxima must be the same on every rank"""
    n = sum(len(r["idx"]) for r in results)
    got = dict(maxdisp=results[0]["maxdisp"], maxvel=results[0]["maxvel"])
    for k in FIELDS:
        got[k] = np.empty((n,) + results[0][k].shape[1:])
    for r in results:
        assert (r["maxdisp"], r["maxvel"]) == (got["maxdisp"], got["maxvel"])
        for k in FIELDS:
            got[k][r["idx"]] = r[k]
    return got
