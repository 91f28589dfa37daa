"""gloo tests (world 2, 3, 4) of the sharded PM with a global_analysis hook (MassiveNuLinRespOn, gravpm.cpp:76-85, 308-321, 412-435) and
the hybrid-neutrino deposit mask (gravpm.cpp:84-85, 459-464) on CPU: shenqi_amd/dist.py splits the X step around the all-reduce of the
P(k) sums (powerspectrum_sum, powerspectrum.cpp:53-88) and multiplies every mode by the hook's T[k2] before the Green's function.
The local phases are numpy stand-ins (NuCpuOps below) with the device kernels' semantics."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cpu_ops import CpuOps  # noqa: E402

NPART, NMESH, BOX, G, ASMTH = 16**3, 48, 8.0, 43.0071, 1.5
ALL_TYPES = -1
NO_TYPE2 = ALL_TYPES & ~(1 << 2)


def nu_table(N, amp=0.3, k0=6.0):
    """a factor in the shape of 1 + nu_prefac nu_spline(log k): T = 1 + amp exp(-k2 / k0^2), by integer k2"""
    k2 = np.arange(3 * (N // 2) ** 2 + 1, dtype=np.float64)
    return 1.0 + amp * np.exp(-k2 / k0**2)


def _kint(N):
    return np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N)


def _invsinc2(k, N):
    t = k * np.pi / N
    s = np.where(np.abs(t) < 1e-5, 1.0 - t**2 / 6 + t**4 / 120, np.sin(t) / np.where(t == 0, 1.0, t))
    return 1.0 / (s * s)


def mode_sums(dk, kx, ky, kz, N):
    """powerspectrum_add_mode (gravpm.cpp:323-356) over the given half-spectrum modes: the raw sums (kk, power, nmodes, Norm)"""
    k2 = kx * kx + ky * ky + kz * kz
    m = dk.real**2 + dk.imag**2
    f = _invsinc2(kx, N) * _invsinc2(ky, N) * _invsinc2(kz, N)
    binsperunit = (N - 1) / np.log(np.sqrt(3) * N / 2.0)
    sel = k2 > 0
    kint = np.floor(binsperunit * np.log(k2[sel].astype(np.float64)) / 2.0).astype(np.int64)
    ok = kint < N
    w = np.where((kz[sel] == 0) | (kz[sel] == N // 2), 1, 2)[ok]
    kint = kint[ok]
    power = np.bincount(kint, weights=w * m[sel][ok] * f[sel][ok] ** 2, minlength=N)
    kk = np.bincount(kint, weights=w * np.sqrt(k2[sel][ok].astype(np.float64)), minlength=N)
    nmodes = np.bincount(kint, weights=w, minlength=N).astype(np.int64)
    norm = float(m[~sel].sum()) if (~sel).any() else 0.0
    return kk, power, nmodes, norm


def restated_power(rho, N, T=None):
    """the sums of the whole density rfftn(rho) (times T[k2] with a table)"""
    k1 = _kint(N)
    kx, ky, kz = np.meshgrid(k1, k1, np.arange(N // 2 + 1), indexing="ij")
    dk = np.fft.rfftn(rho)
    if T is not None:
        k2 = kx * kx + ky * ky + kz * kz
        dk = dk * np.where(k2 > 0, T[k2], 1.0)
    return mode_sums(dk, kx, ky, kz, N)


def restated_potential(rho, N, T=None, Asmth=ASMTH, G=G, L=BOX):
    """irfftn(rfftn(rho) T green), unscaled: potential_transfer with the neutrino factor in front, zero mode removed"""
    k1 = _kint(N)
    kx, ky, kz = np.meshgrid(k1, k1, np.arange(N // 2 + 1), indexing="ij")
    k2 = kx * kx + ky * ky + kz * kz
    dk = np.fft.rfftn(rho)
    if T is not None:
        dk = dk * np.where(k2 > 0, T[k2], 1.0)
    asmth2 = ((2 * np.pi) * Asmth / N) ** 2
    f = _invsinc2(kx, N) * _invsinc2(ky, N) * _invsinc2(kz, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = (-G / (np.pi * L)) * (np.exp(-k2 * asmth2) / k2) * f * f
    fac[k2 == 0] = 0.0
    return np.fft.irfftn(dk * fac, s=(N, N, N), axes=(0, 1, 2), norm="forward")


def assert_sums_close(got, want, rtol):
    """nmodes as integers; kk, power and Norm relative to their largest entry"""
    kk, pw, nm, norm = got
    wkk, wpw, wnm, wnorm = want
    assert np.array_equal(np.asarray(nm, np.int64), np.asarray(wnm, np.int64))
    assert np.abs(kk - wkk).max() <= rtol * np.abs(wkk).max()
    assert np.abs(pw - wpw).max() <= rtol * np.abs(wpw).max()
    assert abs(norm - wnorm) <= rtol * abs(wnorm)


class NuCpuOps(CpuOps):
    """CpuOps with a deposit that honours a type mask and the split Green's step of the torch route: the P(k) sums of this rank's
    transposed spectrum [y_l][z'][x] and a factor table in front of the Green's function"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.types, self.mask = None, ALL_TYPES

    def set_particles(self, posm_all, nlocal, keep_tree=False, types=None):
        super().set_particles(posm_all, nlocal)
        self.types = None if types is None else types.numpy().astype(np.int64)

    def set_deposit_types(self, mask):
        self.mask = mask

    def deposit(self, plane0, nxl, ghosts=1):
        if self.mask == ALL_TYPES:
            return super().deposit(plane0, nxl, ghosts)
        keep = ((self.mask >> self.types[: self.nlocal]) & 1).astype(bool)
        posm, nlocal = self.posm, self.nlocal
        self.posm, self.nlocal = posm[: nlocal][keep], int(keep.sum())
        try:
            return super().deposit(plane0, nxl, ghosts)
        finally:
            self.posm, self.nlocal = posm, nlocal

    def _sums(self, spec_t, y0, nyl, T=None):
        N = self.N
        k1 = _kint(N)
        ky, kz, kx = np.meshgrid(k1[y0:y0 + nyl], np.arange(N // 2 + 1), k1, indexing="ij")
        dk = spec_t.numpy()
        if T is not None:
            k2 = kx * kx + ky * ky + kz * kz
            dk = dk * np.where(k2 > 0, T[k2], 1.0)
        return mode_sums(dk, kx, ky, kz, N)

    def green_forward(self, spec_t, y0, nyl):
        return self._sums(spec_t, y0, nyl)

    def green_finish(self, spec_t, y0, nyl, table=None, measure=False):
        sums = self._sums(spec_t, y0, nyl, table) if measure else None
        if table is not None:
            N = self.N
            k1 = _kint(N)
            ky, kz, kx = np.meshgrid(k1[y0:y0 + nyl], np.arange(N // 2 + 1), k1, indexing="ij")
            k2 = kx * kx + ky * ky + kz * kz
            spec_t.numpy()[...] *= np.where(k2 > 0, table[k2], 1.0)
        self.green(spec_t, y0, nyl)
        return sums


def _global_particles():
    import orc
    import common as cm
    pos = cm.random_positions(orc.boost_mt19937_uniform(0, 3 * NPART), NPART)
    return np.concatenate([pos, np.ones((NPART, 1))], axis=1)


def _global_types():
    t = np.ones(NPART, dtype=np.int64)
    t[::8] = 2                                            # hybrid-neutrino tracers
    return t


def _worker(rank, world, initfile, outdir):
    os.environ["OMP_NUM_THREADS"] = "2"
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        from shenqi_amd import dist as sd
        comm = sd.Comm()
        posm_g, types_g = _global_particles(), _global_types()
        mine = torch.from_numpy(posm_g[rank::world].copy())
        decomp = sd.SlabDecomp(comm, NMESH, BOX)
        local, ltypes = sd.exchange_to_owner(comm, decomp, mine, types=torch.from_numpy(types_g[rank::world].copy()))
        nloc = local.shape[0]
        T = nu_table(NMESH)
        seen = []

        def analysis(kk, power, nmodes, norm):
            seen.append((kk.copy(), power.copy(), nmodes.copy(), norm))
            return T

        out = {}
        for case, mask in (("nu", ALL_TYPES), ("masked", NO_TYPE2)):
            ops = NuCpuOps(NMESH, BOX, ASMTH, G)
            ops.set_deposit_scale(comm.allreduce_sum(float(local[:, 3].sum())))
            ops.set_particles(local, nloc, types=ltypes)
            ops.set_deposit_types(mask)
            pm = sd.SlabPM(comm, NMESH, BOX, ASMTH, G, ops)
            pm.force(analysis=analysis, measure_power=True)
            g, p = ops.results(nloc)
            out[case] = np.concatenate([local.numpy(), ltypes.numpy()[:, None].astype(np.float64), g, p[:, None]], axis=1)
            out[case + "_power"] = pm.power
            out[case + "_finish"] = pm.power_finish
        # the hook saw the reduced density sums, the ones kept on the object
        assert len(seen) == 2
        for a, b in zip(seen[0], out["nu_power"]):
            assert np.array_equal(a, b)
        np.save(os.path.join(outdir, "r%d.npy" % rank), np.array([out], dtype=object), allow_pickle=True)
    finally:
        dist.destroy_process_group()


def _full_rho(posm, types=None, mask=ALL_TYPES):
    """the fixed-point CIC density of the whole set (the deposit the sharded ranks add up), as one CpuOps rank"""
    ops = NuCpuOps(NMESH, BOX, ASMTH, G)
    ops.set_deposit_scale(float(posm[:, 3].sum()))
    ops.set_particles(torch.from_numpy(posm), len(posm), types=None if types is None else torch.from_numpy(types))
    ops.set_deposit_types(mask)
    return ops, ops.to_real(ops.deposit(0, NMESH)).numpy()[:, :, :NMESH]


def _forces(ops, phi):
    ext = np.zeros((NMESH, NMESH, NMESH + 2))
    ext[:, :, :NMESH] = phi
    ops.readout(torch.from_numpy(ext), 0, NMESH)
    return ops.results(ops.nlocal)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_sharded_pm_neutrino_sums_table_and_mask_gloo(world):
    """Per rank count: the reduced sums are the same on every rank and equal the sums of the whole density (nmodes exactly); the
    forces are the readout of irfftn(rfftn(rho) T green); the finish's sums are those of T rfftn(rho).  Masked case: the Types travel
    with their rows through exchange_to_owner and the driver hands them to its ops; which rows the mask leaves out is the stand-in's
    deposit here (the library's masked slab deposits are checked on the GPU, test_gpu_dist_neutrino.py), and every particle, Type 2
    too, is still read out."""
    posm_g, types_g = _global_particles(), _global_types()
    T = nu_table(NMESH)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, os.path.join(tmp, "init"), tmp), nprocs=world, join=True)
        outs = [np.load(os.path.join(tmp, "r%d.npy" % r), allow_pickle=True)[0] for r in range(world)]
    key = {tuple(p): i for i, p in enumerate(map(tuple, posm_g[:, :3]))}
    for case, mask in (("nu", ALL_TYPES), ("masked", NO_TYPE2)):
        ops, rho = _full_rho(posm_g, types_g, mask)
        for which in ("_power", "_finish"):
            for o in outs[1:]:
                for a, b in zip(o[case + which], outs[0][case + which]):
                    assert np.array_equal(a, b)
        assert_sums_close(outs[0][case + "_power"], restated_power(rho, NMESH), 1e-11)
        assert_sums_close(outs[0][case + "_finish"], restated_power(rho, NMESH, T), 1e-11)
        g0, p0 = _forces(ops, restated_potential(rho, NMESH, T))
        rows = np.concatenate([o[case] for o in outs])
        idx = np.array([key[tuple(p)] for p in rows[:, :3]])
        assert len(idx) == NPART and len(set(idx.tolist())) == NPART
        assert np.array_equal(rows[:, 4].astype(np.int64), types_g[idx])         # types travelled with their rows
        assert np.abs(rows[:, 5:8] - g0[idx]).max() <= 1e-10 * np.abs(g0).max()
        assert np.abs(rows[:, 8] - p0[idx]).max() <= 1e-10 * np.abs(p0).max()
        assert np.abs(rows[rows[:, 4] == 2, 5:8]).max() > 0                     # tracers still receive GravPM
