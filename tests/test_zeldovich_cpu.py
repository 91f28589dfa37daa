"""The Zel'dovich displacements without a GPU: the library's host-only seed table against the numpy restatement (zeldovich_restated.py),
and the restatement itself pinned by what does not depend on the reference's output - the engine by the C++ standard's value, the
field by the structure the reference relies on.  There is no reference output for gaussian_fill (pmesh.h needs boost): the restatement
is line by line and otherwise unpinned."""
import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import orc
import zeldovich_restated as zr


@pytest.mark.parametrize("N", [8, 16, 24, 48])
def test_seed_table_matches_restatement(N):
    """SETSEED's tables [0][0] and [1][1], entry for entry, for a few seeds; and [1][1][i, j] = [0][0][-i, -j], which the one-generator
    fill relies on"""
    for seed in (0, 1, 181170, 2**31 - 1):
        t00, t11 = sq.zeldovich_seed_table(N, seed)
        ref = zr.seed_table(N, seed)
        assert np.array_equal(t00, ref[0][0]) and np.array_equal(t11, ref[1][1])
        idx = (N - np.arange(N)) % N
        assert np.array_equal(t11, t00[np.ix_(idx, idx)])
        assert t00.max() < 0x7FFFFFFF and len(np.unique(t00)) > N * N // 2


def test_seed_table_bad_arguments():
    t = np.zeros((7, 7), dtype=np.uint32)
    assert capi.hip.shq_zeldovich_seed_table(7, 1, capi.ptr(t), capi.ptr(t)) == 1
    assert capi.hip.shq_zeldovich_seed_table(8, 1, None, None) == 1


def test_engine_standard_value():
    """[rand.predef]: the 10000th consecutive invocation of a default-constructed mt19937 (seed 5489) produces 4123659995"""
    raw = zr.raw_outputs(zr.init_genrand([5489]), 10000)
    assert int(raw[0, 9999]) == 4123659995
    # and the variate is the repository's reading of boost's distribution
    assert np.array_equal(raw[0, :100].astype(np.float64) / 4294967296.0, orc.boost_mt19937_uniform(5489, 100))


def test_redraw_shifts_the_stream():
    """a state whose second output is 0 (mt[1] = mt[2] = mt[398] = 0 before the twist; tempering keeps 0): the first SAMPLE redraws its
    ampl, and every later SAMPLE of that generator starts one draw later"""
    st = zr.init_genrand([12345])
    st[0, [1, 2, 398]] = 0
    raw = zr.raw_outputs(st, 64).astype(np.float64)[0] / 4294967296.0
    assert raw[1] == 0 and raw[2] != 0
    pairs = zr.sample_pairs(st, 20)[0]
    assert pairs[0, 0] == raw[0] * 2 * np.pi and pairs[0, 1] == raw[2]
    assert np.array_equal(pairs[1:, 0], raw[3:3 + 2 * 9:2] * 2 * np.pi) and np.array_equal(pairs[1:, 1], raw[4:4 + 2 * 9:2])


def _complete(half, N):
    """the full complex cube of a half spectrum [x][y][z'] by Hermitian symmetry"""
    full = np.zeros((N, N, N), dtype=np.complex128)
    full[:, :, : N // 2 + 1] = half
    idx = (N - np.arange(N)) % N
    for z in range(N // 2 + 1, N):
        full[:, :, z] = np.conj(half[np.ix_(idx, idx)][:, :, N - z])
    return full


@pytest.mark.parametrize("N", [8, 16])
def test_field_structure(N):
    f = zr.fill_gaussian(N, 9281)
    idx = (N - np.arange(N)) % N
    # Hermitian on the k = 0 and k = N / 2 planes, exactly: the conjugate columns take the same samples
    for k in (0, N // 2):
        assert np.array_equal(f[:, :, k], np.conj(f[np.ix_(idx, idx)][:, :, k]))
    assert f[0, 0, 0] == 0
    for i in (0, N // 2):
        for j in (0, N // 2):
            for k in (0, N // 2):
                assert f[i, j, k].imag == 0
    # a real field: the completed cube's inverse transform has an imaginary part at rounding level
    real = np.fft.ifftn(_complete(f, N)) * N**3
    assert np.abs(real.imag).max() < 1e-12 * np.abs(real.real).max()
    # |ampl| <= sqrt(32 ln 2)
    assert np.abs(f).max() <= np.sqrt(32 * np.log(2))
    # any split of the columns into ranges gives the same field
    rng = np.random.default_rng(N)
    cuts = np.sort(rng.choice(np.arange(1, N * N), 3, replace=False))
    parts = sum(zr.fill_gaussian(N, 9281, columns=c) for c in np.split(np.arange(N * N), cuts))
    assert np.array_equal(parts, f)
    # UnitaryAmplitude: |mode| = 1.  Not at the eight self-conjugate modes: pmesh.h:160-165 keeps ampl * cos(phase) there and drops the
    # imaginary part, so they are real with |mode| = |cos(phase)| <= 1 (and the zero mode is 0).  InvertPhase: every mode negated
    u = zr.fill_gaussian(N, 9281, UnitaryAmplitude=1)
    a = np.abs(u)
    sc = np.ix_((0, N // 2), (0, N // 2), (0, N // 2))
    assert np.all(a[sc] <= 1) and np.all(u[sc].imag == 0)
    a[sc] = 1
    assert np.abs(a - 1).max() < 4e-16
    assert np.abs(np.angle(u[f != 0] / f[f != 0])).max() < 1e-15
    inv = zr.fill_gaussian(N, 9281, InvertPhase=1)
    assert np.abs(inv + f).max() < 8 * np.finfo(float).eps * np.sqrt(32 * np.log(2))
    # another seed gives another field
    assert not np.array_equal(zr.fill_gaussian(N, 9282), f)


@pytest.mark.parametrize("N", [8, 16])
def test_meshes_sum_to_zero(N):
    """the fill zeroes the zero mode and the transfers leave it alone: every real mesh sums to zero at rounding level (over the whole
    mesh: a lattice of Ngrid = Nmesh / 2 also picks up the Nyquist modes)"""
    L = 25.0
    delta = zr.tabulate_k2(lambda k: 2.0 * k**-1.2, N, L)
    growth = zr.tabulate_k2(lambda k: 1.0 + 0.1 * k, N, L)
    spec = zr.reference_layout(zr.fill_gaussian(N, 77))
    meshes = zr.transfer_meshes(spec, N, L, delta, growth)
    assert len(meshes) == 7
    for m in meshes:
        assert np.abs(m).max() > 0
        assert abs(m.sum()) < 1e-12 * np.abs(m).sum()


def test_host_helpers():
    """setup_grid / idgen_* and the table helper of the Python mirror against the restatement's"""
    g = sq.IDGenerator(6, 30.0)
    pos, mass = sq.setup_grid(g, 2.5, 0.25)
    assert np.array_equal(pos, zr.idgen_positions(6, 30.0, 2.5)) and np.all(mass == 0.25) and len(pos) == 216
    ids = sq.idgen_create_id_from_index(g, np.arange(216))
    assert np.array_equal(ids, np.arange(1, 217, dtype=np.uint64))
    f = lambda k: 3.0 * k / (1.0 + k * k)      # + - * / only: the same bits from a Python float and from a numpy array
    assert np.array_equal(sq.tabulate_by_k2(f, 8, 7.0), zr.tabulate_k2(f, 8, 7.0))


def test_factor_tables():
    """shq_zeldovich_factor_tables (host only) against the expressions of density_transfer / disp_transfer"""
    N, L = 16, 7.0
    delta = zr.tabulate_k2(lambda k: 3.0 * k / (1.0 + (k / 2.0) ** 3), N, L)
    growth = zr.tabulate_k2(lambda k: 1.0 + 0.1 * k, N, L)
    n = len(delta)
    dens, disp, vel = np.zeros(n), np.zeros(n), np.zeros(n)
    capi.check(capi.hip.shq_zeldovich_factor_tables(N, L, capi.ptr(delta), capi.ptr(growth), capi.ptr(dens), capi.ptr(disp), capi.ptr(vel)))
    k2 = np.arange(1, n)
    r2 = (1.0 / N) * (1.0 / N)
    assert np.allclose(dens[1:], np.exp(-k2 * r2) * (delta[1:] / np.sqrt(L * L * L)), rtol=4e-16, atol=0)
    assert np.array_equal(disp[1:], 1.0 / (2 * np.pi) / np.sqrt(L) / k2 * delta[1:])
    assert np.array_equal(vel[1:], 1.0 / (2 * np.pi) / np.sqrt(L) / k2 * growth[1:])
    assert dens[0] == 0 and disp[0] == 0 and vel[0] == 0
