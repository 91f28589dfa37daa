"""A numpy restatement of glass making (glass_evolve, libgenic/glass.cpp:76-360) for one rank, written from reading the reference:
petapm's CIC deposit and readout (pm_iterate_one, petapm.cpp:1132-1183), the transfers of glass.cpp:285-351, both power additions
(measure_power_spectrum and potential_transfer through powerspectrum_add_mode, gravpm.cpp:323-376), glass_stats, and
powerspectrum_sum's tail (powerspectrum.cpp:71-87).

Storage is ic_part_data's (allvars.h:8-16): float64 Pos, float32 Vel, Disp and Mass.  The rounding points are what C++ makes of the
reference's expressions:
  Disp[k] += weight * mesh[0]              float64 sum rounded to float32 after each of the eight connections
  Vel[d] += (Disp[d] - Vel[d]) * hdt       the difference is a float32 subtraction; the product and the sum are float64; rounded to float32
  Pos[d] += Vel[d] * dt                    float64
Positions are never wrapped: cell = floor(Pos / CellSize), residual from the unwrapped quotient, index modulo Nmesh.
The transforms are the unscaled ones: rfftn, and irfftn * Nmesh^3.  Meshes and spectra are dense [x][y][z] / [x][y][z']."""
import math

import numpy as np

import zeldovich_restated as zr

DT = math.pi / 2
HDT = 0.5 * DT


def cic_cells(pos, N, BoxSize):
    """pm_iterate_one's iCell (before the periodic fold) and Res"""
    cellsize = BoxSize / N
    tmp = np.asarray(pos, dtype=np.float64) / cellsize
    cell = np.floor(tmp)
    return cell.astype(np.int64), tmp - cell


def connections(cell, res, N):
    """the eight (index tuple, weight) of a particle set, in connection order: offset along axis k is (connection >> k) & 1"""
    for connection in range(8):
        weight = np.ones(len(cell))
        idx = []
        for k in range(3):
            off = (connection >> k) & 1
            idx.append((cell[:, k] + off) % N)
            weight = weight * (res[:, k] if off else (1 - res[:, k]))
        yield tuple(idx), weight


def deposit(pos, mass, N, BoxSize):
    """put_particle_to_mesh: mesh += weight * Mass"""
    cell, res = cic_cells(pos, N, BoxSize)
    mesh = np.zeros((N, N, N))
    m = np.asarray(mass, dtype=np.float32).astype(np.float64)
    for idx, weight in connections(cell, res, N):
        np.add.at(mesh, idx, weight * m)
    return mesh


def gather_f32(mesh, pos, N, BoxSize):
    """readout_force_*: float32 Disp from 0, the float64 sum rounded to float32 after every connection"""
    cell, res = cic_cells(pos, N, BoxSize)
    acc = np.zeros(len(cell), dtype=np.float32)
    for idx, weight in connections(cell, res, N):
        acc = (acc.astype(np.float64) + weight * mesh[idx]).astype(np.float32)
    return acc


def kgrid(N):
    k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N).astype(np.int64)
    kx, ky, kz = np.meshgrid(k1, k1, k1[: N // 2 + 1], indexing="ij")
    return k1, kx, ky, kz, kx * kx + ky * ky + kz * kz


def diff_kernel(w):
    return 1 / 6.0 * (8 * math.sin(w) - math.sin(2 * w))


def force_factor(N, BoxSize):
    """force_transfer's fac per mesh index"""
    k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N)
    return np.array([-1 * diff_kernel(int(k) * (2 * math.pi / N)) * (N / BoxSize) for k in k1])


def total_mass(mass):
    """totmass += Mass: float64, in particle order"""
    m = np.asarray(mass, dtype=np.float32).astype(np.float64)
    return float(np.cumsum(m)[-1])


def pot_factor(BoxSize, totmass):
    return -1 * (-1) * math.pow(2 * math.pi / BoxSize, -2) / totmass


def sinc_table(N):
    """1 / sinc_unnormed(kpos pi / Nmesh)^2 per mesh index (measure_power_spectrum)"""
    out = np.zeros(N)
    for i in range(N):
        k = i if i <= N // 2 else i - N
        tmp = (k * math.pi) / N
        if -1e-5 < tmp < 1e-5:
            x2 = tmp * tmp
            s = 1.0 - x2 / 6.0 + x2 * x2 / 120.0
        else:
            s = math.sin(tmp) / tmp
        out[i] = 1.0 / (s * s)
    return out


def power_sums(spec, N, invwindow):
    """powerspectrum_add_mode over every mode of the half spectrum with the given invwindow array: (kk, power, nmodes, norm), size Nmesh"""
    size = N
    _, kx, ky, kz, k2 = kgrid(N)
    m = spec.real * spec.real + spec.imag * spec.imag
    norm = float(m[0, 0, 0])
    binsperunit = (size - 1) / math.log(math.sqrt(3) * N / 2.0)
    nz = k2 > 0
    kint = np.floor(binsperunit * np.log(np.where(nz, k2, 1).astype(np.float64)) / 2.0).astype(np.int64)
    use = nz & (kint < size)
    w = np.where((kz == 0) | (kz == N // 2), 1, 2)
    keff = np.sqrt(k2.astype(np.float64))
    power = np.bincount(kint[use], weights=(w * m * invwindow * invwindow)[use], minlength=size)[:size]
    kk = np.bincount(kint[use], weights=(w * keff)[use], minlength=size)[:size]
    nmodes = np.bincount(kint[use], weights=w[use], minlength=size)[:size].astype(np.int64)
    return kk, power, nmodes, norm


def glass_power(spec, N):
    """what pm->ps holds after one petapm_force of the glass: measure_power_spectrum (deconvolved) plus potential_transfer (invwindow 1)"""
    s = sinc_table(N)
    f = s[:, None, None] * s[None, :, None] * s[None, None, : N // 2 + 1]
    a = power_sums(spec, N, f)
    b = power_sums(spec, N, np.ones_like(f))
    return a[0] + b[0], a[1] + b[1], a[2] + b[2], b[3]


def force_meshes(pos, mass, N, BoxSize):
    """the density spectrum and the three real force meshes"""
    spec = np.fft.rfftn(deposit(pos, mass, N, BoxSize))
    _, kx, ky, kz, k2 = kgrid(N)
    nz = k2 > 0
    fac = pot_factor(BoxSize, total_mass(mass)) * (1.0 / np.where(nz, k2, 1)) * 1.0 * 1.0
    pot = np.where(nz, spec * fac, 0.0)
    ff = force_factor(N, BoxSize)
    meshes = []
    for axis, kidx in enumerate(np.meshgrid(np.arange(N), np.arange(N), np.arange(N // 2 + 1), indexing="ij")):
        fa = ff[kidx]
        e = (-pot.imag * fa) + 1j * (pot.real * fa)
        meshes.append(np.fft.irfftn(e, s=(N, N, N), axes=(0, 1, 2)) * float(N) ** 3)
    return spec, meshes


def glass_force(pos, mass, N, BoxSize, spectrum=False):
    """glass_force: Disp zeroed, the PM force gathered into it.  Returns (Disp float32 [n][3], meshes, raw power sums or None)"""
    spec, meshes = force_meshes(pos, mass, N, BoxSize)
    disp = np.stack([gather_f32(meshes[k], pos, N, BoxSize) for k in range(3)], axis=1)
    return disp, meshes, (glass_power(spec, N) if spectrum else None)


def kick(vel, disp):
    dv = (disp.astype(np.float32) - vel.astype(np.float32)).astype(np.float32)   # float - float
    return (vel.astype(np.float64) + dv.astype(np.float64) * HDT).astype(np.float32)


def drift(pos, vel):
    return pos + vel.astype(np.float64) * DT


def glass_stats(disp, vel):
    n = float(len(disp))
    d, v = disp.astype(np.float64), vel.astype(np.float64)
    return math.sqrt(float((d * d).sum()) / n), math.sqrt(float((v * v).sum()) / n)


def glass_evolve(pos, vel, mass, N, BoxSize, nsteps, spectrum=False):
    """glass_evolve.  Returns dict(Pos, Vel, Disp, steps, spectra, disp0): disp0 is the opening force"""
    pos = np.array(pos, dtype=np.float64)
    vel = np.array(vel, dtype=np.float32)
    t_x = t_v = t_f = 0.0
    disp, _, _ = glass_force(pos, mass, N, BoxSize)
    disp0 = disp.copy()
    steps, spectra = [], []
    for _ in range(nsteps):
        vel = kick(vel, disp)
        t_x += HDT
        pos = drift(pos, vel)
        t_v += DT
        disp, _, ps = glass_force(pos, mass, N, BoxSize, spectrum)
        t_f = t_x
        vel = kick(vel, disp)
        t_x += HDT
        fs, vs = glass_stats(disp, vel)
        steps.append(dict(t_f=t_f, t_v=t_v, t_x=t_x, force_std=fs, vel_std=vs))
        spectra.append(ps)
    return dict(Pos=pos, Vel=vel, Disp=disp, steps=steps, spectra=spectra, disp0=disp0)


def setup_positions(Ngrid, BoxSize, shift, seed):
    """setup_glass's loop (glass.cpp:56-66): one serial mt19937(seed), uniform_real_distribution<double>(0, 1) read as raw / 2^32 with a
    redraw unless the result is below 1 (which a 32-bit raw / 2^32 always is), three draws per particle in k order"""
    n = Ngrid**3
    u = zr.raw_outputs(zr.init_genrand([seed & 0xFFFFFFFF]), 3 * n)[0].astype(np.float64) / 4294967296.0
    pos = zr.idgen_positions(Ngrid, BoxSize)
    rand = BoxSize / Ngrid * 3 * (u.reshape(n, 3) - 0.5)
    return pos + (shift + rand)


def finish_power(size, BoxSize_in_MPC, kk, power, nmodes, norm):
    """powerspectrum_sum's tail on one rank's sums: the non-empty bins, moved to the front"""
    kk, power, nmodes = np.array(kk, dtype=np.float64), np.array(power, dtype=np.float64), np.array(nmodes, dtype=np.int64)
    keep = nmodes[:size] != 0
    P = power[:size][keep] / nmodes[:size][keep]
    P = P / norm
    K = kk[:size][keep] / nmodes[:size][keep]
    K = K * (2 * math.pi / BoxSize_in_MPC)
    P = P * math.pow(BoxSize_in_MPC, 3.0)
    return K, P, nmodes[:size][keep]
