"""Shared pieces of the sharded glass tests (test_dist_glass_cpu.py, test_gpu_dist_glass.py): the particles (setup_glass's positions,
some pushed out of the box on both sides), the deals, a numpy stand-in for DistGlass's ops built on glass_restated, the per-rank run
with its assembly, and the comparison of one step against the restatement at the bars of test_gpu_glass.py."""
import functools
import math

import numpy as np
import torch

import glass_restated as gr
from test_gpu_glass import BAR, L, _disp_bar, _input, _ulp32  # noqa: F401

FIELDS = ("Pos", "Vel", "Disp")


@functools.lru_cache(maxsize=None)
def particles(Ngrid, seed, outside=True):
    pos = _input(Ngrid, seed, outside)
    pos.setflags(write=False)
    return pos


def deal(n, size, how):
    """which rank holds which particle: 1 round-robin, 2 blocks in reversed rank order (neither is by slab)"""
    return np.arange(n) % size if how == 1 else size - 1 - np.arange(n) * size // n


def owners(pos, N, P, box=L):
    """the rank that owns each particle: its CIC base plane, floor(x / cell) modulo N as cic_setup takes it, over equal slabs"""
    return (np.floor(pos[:, 0] / (box / N)).astype(np.int64) % N) // (N // P)


def slab_k(N, y0, nyl):
    k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N).astype(np.int64)
    kx, ky, kz = np.meshgrid(k1, k1[y0:y0 + nyl], k1[:N // 2 + 1], indexing="ij")
    return kx, ky, kz, kx * kx + ky * ky + kz * kz


def slab_power(spec, N, y0, nyl):
    """both power additions of a glass force (glass_restated.glass_power) on rows [y0, y0 + nyl) of [x][y][z']: (kk, power, nmodes,
    norm); norm is 0 on a slab without the zero mode"""
    _, _, kz, k2 = slab_k(N, y0, nyl)
    s = gr.sinc_table(N)
    f = s[:, None, None] * s[None, y0:y0 + nyl, None] * s[None, None, :N // 2 + 1]
    m = spec.real * spec.real + spec.imag * spec.imag
    norm = float(m[0, 0, 0]) if y0 == 0 else 0.0
    binsperunit = (N - 1) / math.log(math.sqrt(3) * N / 2.0)
    nz = k2 > 0
    kint = np.floor(binsperunit * np.log(np.where(nz, k2, 1).astype(np.float64)) / 2.0).astype(np.int64)
    use = nz & (kint < N)
    w = np.where((kz == 0) | (kz == N // 2), 1, 2)
    keff = np.sqrt(k2.astype(np.float64))
    power = np.bincount(kint[use], weights=(w * m * f * f + w * m)[use], minlength=N)[:N]
    kk = np.bincount(kint[use], weights=(2 * (w * keff))[use], minlength=N)[:N]
    nmodes = np.bincount(kint[use], weights=(2 * w)[use], minlength=N)[:N].astype(np.int64)
    return kk, power, nmodes, norm


def slab_transfer(spec, N, box, totmass, y0, nyl, axis):
    """potential_transfer and force_transfer of one axis in the restatement's operation order on rows [y0, y0 + nyl) of [x][y][z']"""
    _, _, _, k2 = slab_k(N, y0, nyl)
    nz = k2 > 0
    fac = gr.pot_factor(box, totmass) * (1.0 / np.where(nz, k2, 1)) * 1.0 * 1.0
    pot = np.where(nz, spec * fac, 0.0)
    idx = np.meshgrid(np.arange(N), np.arange(y0, y0 + nyl), np.arange(N // 2 + 1), indexing="ij")[axis]
    fa = gr.force_factor(N, box)[idx]
    return (-pot.imag * fa) + 1j * (pot.real * fa)


class RestatedGlassOps:
    """DistGlass's ops in numpy from the restatement's pieces, on the torch.fft route.  The deposit adds the integers the device adds
    (round(weight * Mass * 2^(61 - exp))), so the stand-in's meshes do not depend on who holds which particle either."""
    device = torch.device("cpu")

    def pitch(self, N):
        return 0

    def full(self, shape, value, dtype):
        return torch.full(shape, value, dtype=dtype)

    def tables(self, N, box, totmass):
        self.box, self.totmass = box, totmass

    def planes(self, N, box, pos):
        return torch.from_numpy((np.floor(pos.numpy()[:, 0] / (box / N)).astype(np.int64) % N).astype(np.int32))

    def _window(self, pos, N, box, plane0, nxl, nalloc):
        cell, res = gr.cic_cells(pos, N, box)
        assert ((cell[:, 0] % N - plane0) % N < nxl).all(), "a particle outside this rank's slab"
        for idx, weight in gr.connections(cell, res, N):
            ix = (idx[0] - plane0) % N
            assert (ix < nalloc).all()
            yield (ix, idx[1], idx[2]), weight

    def deposit(self, N, box, pos, mass, exp, plane0, nxl, buf):
        b = buf.numpy()
        b[...] = 0
        m = mass.numpy().astype(np.float64)
        scale = math.ldexp(1.0, 61 - exp)
        for idx, weight in self._window(pos.numpy(), N, box, plane0, nxl, b.shape[0]):
            np.add.at(b, idx, np.rint(weight * m * scale).astype(np.int64))

    def to_real(self, mesh_i, exp):
        return mesh_i.to(torch.float64) * math.ldexp(1.0, exp - 61)

    def power(self, N, spec, y0, nyl, sums):
        kk, power, nmodes, norm = slab_power(spec.numpy(), N, y0, nyl)
        s = sums.numpy()
        s[:N] += power
        s[N:2 * N] += kk
        s[2 * N:3 * N].view(np.int64)[:] += nmodes
        if y0 == 0:
            s[3 * N] = norm

    def transfer(self, N, spec, y0, nyl, axis):
        return torch.from_numpy(slab_transfer(spec.numpy(), N, self.box, self.totmass, y0, nyl, axis))

    def gather(self, N, box, pos, window, plane0, nxl, disp, axis):
        w = window.numpy()
        acc = np.zeros(pos.shape[0], dtype=np.float32)
        for idx, weight in self._window(pos.numpy(), N, box, plane0, nxl, w.shape[0]):
            acc = (acc.astype(np.float64) + weight * w[idx]).astype(np.float32)
        disp.numpy()[:, axis] = acc

    def particles(self, pos, vel, disp, ending, beginning):
        p, v, d = pos.numpy(), vel.numpy(), disp.numpy()
        sums = [0.0, 0.0]
        if ending:
            v[...] = gr.kick(v, d)
            sums = [float((d.astype(np.float64) ** 2).sum()), float((v.astype(np.float64) ** 2).sum())]
        if beginning:
            v[...] = gr.kick(v, d)
            p[...] = gr.drift(p, v)
        return sums


def run_rank(comm, ops, N, pos, mass, how=1, holder=None, calls=(14,), spectra=True, vel=None, box=L, drv=None):
    """one rank's calls on its share of the particles: calls = the nsteps of successive evolve calls, each from the state the one
    before returned.  Returns dict(idx, outs = one dict per call with the counters, error)"""
    from shenqi_amd import dist as sd
    who = deal(len(pos), comm.size, how) if holder is None else holder
    idx = np.flatnonzero(who == comm.rank)
    try:
        drv = sd.DistGlass(comm, N, box, ops) if drv is None else drv
    except ValueError as e:
        return dict(error=str(e), constructor=True)
    p, v, m = pos[idx], (None if vel is None else vel[idx]), (mass if np.isscalar(mass) else mass[idx])
    outs = []
    for nsteps in calls:
        try:
            out = drv.evolve(p, v, m, nsteps, spectra=spectra)
        except ValueError as e:
            return dict(error=str(e), nalltoall=drv.nalltoall, idx=idx, outs=outs)
        out.update(rows_sent=drv.rows_sent, rehomed=list(drv.rehomed), nalltoall=drv.nalltoall)
        outs.append(out)
        p, v = out["Pos"], out["Vel"]
    return dict(idx=idx, outs=outs)


def assemble(results, call=0):
    """call `call` of every rank as one result in the global particle order; steps and spectra must be the same on every rank"""
    n = sum(len(r["idx"]) for r in results)
    first = results[0]["outs"][call]
    got = {k: np.empty((n, 3), dtype=first[k].dtype) for k in FIELDS}
    got["steps"] = first["steps"]
    got["rehomed"] = np.sum([r["outs"][call]["rehomed"] for r in results], axis=0).astype(np.int64)
    for k in ("kk", "power", "nmodes", "norm"):
        if k in first:
            got[k] = first[k]
    for r in results:
        o = r["outs"][call]
        assert o["steps"] == first["steps"]
        for k in ("kk", "power", "nmodes", "norm"):
            if k in first:
                assert np.array_equal(o[k], first[k]), k
        for k in FIELDS:
            got[k][r["idx"]] = o[k]
    return got


def compare_step(pos, vel, mass, out, N, tag, box=L):
    """test_every_step_from_the_device_state's comparison of ONE step: the state (pos, vel) before it, the driver's result `out` of a
    one-step call with spectra.  The closing force is restated at the driver's own drifted positions and the closing kick takes the
    driver's Disp, so the comparison holds no derivative of the force field.  Returns the errors over their bars."""
    n = len(pos)
    mass = np.full(n, mass, dtype=np.float32) if np.isscalar(mass) else mass
    d0, m0, _ = gr.glass_force(pos, mass, N, box)
    bar0 = _disp_bar(m0)
    v1 = gr.kick(vel, d0)
    bar_v1 = bar0 * gr.HDT + _ulp32(v1)
    p1 = gr.drift(pos, v1)
    bar_p = bar_v1 * gr.DT + 2 * float(np.spacing(np.abs(p1).max()))
    e_p = np.abs(out["Pos"] - p1).max()
    assert e_p <= bar_p, (tag, "Pos", e_p, bar_p)
    d1, m1, ps = gr.glass_force(out["Pos"], mass, N, box, spectrum=True)
    bar1 = _disp_bar(m1)
    e_d = np.abs(out["Disp"].astype(np.float64) - d1).max()
    assert out["Disp"].dtype == np.float32 and e_d <= bar1, (tag, "Disp", e_d, bar1)
    v2 = gr.kick(v1, out["Disp"])
    bar_v2 = bar_v1 * abs(1 - gr.HDT) + 2 * _ulp32(v2)
    e_v = np.abs(out["Vel"].astype(np.float64) - v2).max()
    assert out["Vel"].dtype == np.float32 and e_v <= bar_v2, (tag, "Vel", e_v, bar_v2)
    # statistics on the driver's own Disp and Vel: 3 n non-negative terms in any order
    fs, vs = gr.glass_stats(out["Disp"], out["Vel"])
    tol = 3 * (3 * n) * 2.0**-53
    st = out["steps"][0]
    assert abs(st["force_std"] / fs - 1) <= tol and abs(st["vel_std"] / vs - 1) <= tol, (tag, st, fs, vs)
    assert (st["t_f"], st["t_v"], st["t_x"]) == (gr.HDT, gr.DT, gr.HDT + gr.HDT)
    # the spectrum of this step's force, restated on the driver's positions
    kk, power, nmodes, norm = ps
    nz = nmodes > 0
    anyorder = 3 * (N**3) * 2.0**-53
    assert np.array_equal(out["nmodes"][0], nmodes) and nmodes.sum() == 2 * (N**3 - 1), tag
    assert np.abs(out["kk"][0][nz] / kk[nz] - 1).max() <= 1e-11 + anyorder, tag
    assert np.abs(out["power"][0][nz] / power[nz] - 1).max() <= 1e-11 + anyorder, tag
    assert not out["power"][0][~nz].any() and abs(out["norm"][0] / norm - 1) <= 1e-11 + anyorder, tag
    return dict(pos=e_p / bar_p, disp=e_d / bar1, vel=e_v / bar_v2)


def restated_owner_changes(pos, vel, mass, N, P, nsteps, box=L):
    """per step of glass_restated.glass_evolve the number of particles whose owner changes in the drift, and the final state"""
    pos, vel = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float32)
    disp, _, _ = gr.glass_force(pos, mass, N, box)
    moved = []
    for _ in range(nsteps):
        vel = gr.kick(vel, disp)
        before = owners(pos, N, P, box)
        pos = gr.drift(pos, vel)
        moved.append(int((owners(pos, N, P, box) != before).sum()))
        disp, _, _ = gr.glass_force(pos, mass, N, box)
        vel = gr.kick(vel, disp)
    return moved, pos
