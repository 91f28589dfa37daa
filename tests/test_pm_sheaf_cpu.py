"""The two-dimensional reduction of tests/pm_sheaf.py against a full three-dimensional numpy PM on the same particles, and the
row coverage of every sheaf the GPU tests use.  Both sides are double precision on the CPU: bounds 1e-12 of the respective maximum."""
import numpy as np
import pytest
import torch

import orc
import pm_sheaf as ps
from cpu_ops import CpuOps

ASMTH, G = 1.5, 43.0071
DIRECTIONS = [(1, 1, 1), (1, -1, 1), (0, 0, 1), (1, 0, 0), (2, 3, 1)]


def full_pm(sh, modefac=None):
    """CpuOps deposit, rfftn, green, unscaled irfftn, readout on the dense N^3 mesh: GravPM, PM potential, the density mesh"""
    N = sh.N
    ops = CpuOps(N, float(N), ASMTH, G)
    ops.set_particles(torch.from_numpy(np.column_stack([sh.pos, sh.mass])), len(sh.pos))
    ops.set_deposit_scale(float(sh.mass.sum()))
    rho = ops.to_real(ops.deposit(0, N))[:, :, :N].numpy()
    spec = np.ascontiguousarray(np.fft.rfftn(rho).transpose(1, 2, 0))          # [y][z'][x], the layout green enumerates
    if modefac is not None:
        k1 = np.where(np.arange(N) <= N // 2, np.arange(N), np.arange(N) - N)
        ky, kz, kx = np.meshgrid(k1, k1[: N // 2 + 1], k1, indexing="ij")
        spec *= modefac[kx**2 + ky**2 + kz**2]
    ops.green(torch.from_numpy(spec), 0, N)
    phi = np.fft.irfftn(spec.transpose(2, 0, 1), s=(N, N, N), axes=(0, 1, 2)) * float(N) ** 3
    ops.readout(torch.from_numpy(np.ascontiguousarray(phi)), 0, N)
    return ops.gravpm, ops.pmpot, rho, phi


@pytest.mark.parametrize("d", DIRECTIONS)
@pytest.mark.parametrize("N", [16, 24, 40, 48])
def test_reduction_equals_the_dense_pm(N, d):
    sh = ps.make_sheaf(N, d, 2 * N, 500, seed=N + 1)
    r, p, q, a, b = ps.frame(d)
    g, pot, rho, phi = full_pm(sh)
    # the deposit is invariant under the shift by d, and the potential mesh is g
    X = np.indices((N, N, N))
    f = ps.reduced_density(sh)
    assert np.array_equal(rho, f[(X[p] - a * X[r]) % N, (X[q] - b * X[r]) % N])
    g2 = ps.reduced_potential(sh, ASMTH, G)
    assert np.abs(phi - g2[(X[p] - a * X[r]) % N, (X[q] - b * X[r]) % N]).max() < 1e-12 * np.abs(phi).max()
    rg, rpot = ps.reduced_reference(sh, ASMTH, G)
    assert np.abs(rg - g).max() < 1e-12 * np.abs(g).max()
    assert np.abs(rpot - pot).max() < 1e-12 * np.abs(pot).max()
    assert np.abs(g[sh.nline_parts:]).max() > 0.1 * np.abs(g).max()            # the probes feel forces of the lines' order
    # with a mode factor
    T = ps.mode_factor(N)
    gT, potT, _, _ = full_pm(sh, T)
    rgT, rpotT = ps.reduced_reference(sh, ASMTH, G, modefac=T)
    assert np.abs(rgT - gT).max() < 1e-12 * np.abs(gT).max()
    assert np.abs(rpotT - potT).max() < 1e-12 * np.abs(potT).max()
    assert np.abs(gT - g).max() > 1e-3 * np.abs(g).max()                       # T is not trivial
    # the P(k) sums
    _, opower, _, onorm = orc.power_spectrum(rho, N)
    power, norm = ps.power_sums(sh)
    assert np.abs(power - opower).max() < 1e-12 * opower.max()
    assert abs(norm - onorm) < 1e-12 * onorm and abs(norm - sh.mass.sum() ** 2) < 1e-12 * norm


def test_shifted_sheaf_is_a_sheaf():
    """the translated load of the GPU tests: the reduction holds for it as it stands"""
    N, d = 24, (1, -1, 1)
    sh = ps.make_sheaf(N, d, 2 * N, 300, seed=5).shifted((N - 3, 7, N - 1))
    g, pot, _, _ = full_pm(sh)
    rg, rpot = ps.reduced_reference(sh, ASMTH, G)
    assert np.abs(rg - g).max() < 1e-12 * np.abs(g).max()
    assert np.abs(rpot - pot).max() < 1e-12 * np.abs(pot).max()


def test_row_coverage_of_the_reduction_is_the_dense_count():
    """row_coverage works from the support of f; here against the rows of the dense mesh"""
    for N, d, nl in [(16, (1, 1, 1), 5), (24, (1, -1, 1), 9), (16, (0, 0, 1), 30), (24, (1, 0, 0), 40), (16, (2, 3, 1), 6)]:
        sh = ps.make_sheaf(N, d, nl, 0, seed=3)
        _, _, rho, _ = full_pm(sh)
        dense = [float((np.abs(rho).sum(axis=k) > 0).mean()) for k in range(3)]
        assert np.allclose(ps.row_coverage(sh), dense, rtol=0, atol=1e-15), (N, d, ps.row_coverage(sh), dense)


def test_row_coverage_of_every_gpu_case():
    """at least 90 % of the mesh rows along each axis hold mass, so that a forward pass that mishandles a zero row - or a
    non-zero one - is seen.  Along an axis direction d itself that takes N^3 particles: asserted at Nmesh 48, and from 768 on
    those rows are the lines' own columns (pm_sheaf.nlines_for) - the case is there for the kz = 0 and N/2 columns and the DC
    lines, which a row that is constant along d excites."""
    cases = ps.gpu_cases() + [(36, d) for d in ps.DIAGONALS] + [(100, d) for d in ps.DIAGONALS]
    assert len(ps.compiled_sizes()) >= 19
    for N, d in cases:
        sh = ps.gpu_case(N, d, nprobes=0)
        cov = ps.row_coverage(sh)
        r = ps.frame(d)[0]
        for k in range(3):
            if k == r and ps.axis_rows_sparse(N, d):
                assert cov[k] >= ps.AXIS_SPARSE_SHARE, (N, d, cov)
            else:
                assert cov[k] >= 0.9, (N, d, cov)
        if d in ps.DIAGONALS:
            assert cov == [1.0, 1.0, 1.0], (N, d, cov)
