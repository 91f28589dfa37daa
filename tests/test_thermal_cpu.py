"""The thermal velocities without a GPU: the restatement (thermal_restated.py) pinned by what does not depend on the reference's output -
the engine by the C++ standard's value and libstdc++'s first outputs, the slopes by scipy's makima, the distribution by the reference's
own gates (libgenic/tests/test_thermal.cpp) - and the library's host-only entries against it."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.integrate import quad
from scipy.interpolate import Akima1DInterpolator

import shenqi_amd as sq
from shenqi_amd import capi
import thermal_restated as tr

ERR_INVALID = 1
# the first three outputs of std::ranlux48(seed) (libstdc++)
FIRST = {0: (23459059301164, 28639057539807, 276846226770426),
         1: (23223501020940, 200574105549927, 178425737289561),
         12345: (118360775523179, 177334856190914, 224501953691856),
         4294967295: (280461857115868, 119442517100906, 257380186664813)}


def test_engine_standard_value_and_first_outputs():
    """[rand.predef]: the 10000th consecutive invocation of a default-constructed ranlux48 (seed 19780503) produces 249142670248501"""
    assert tr.ranlux48_stream(19780503, 10000)[-1] == 249142670248501
    for seed, first in FIRST.items():
        assert tuple(tr.ranlux48_stream(seed, 3)) == first, seed
    # seed 0 stands for the default seed
    assert tr.ranlux48_stream(0, 30) == tr.ranlux48_stream(19780503, 30)
    # the engines advanced together are the serial engine, across three discard blocks
    seeds = list(FIRST) + [2147483563, 2147483564]       # the LCG's modulus: v mod m == 0 starts from 1
    both = tr.Ranlux48(seeds).outputs(40)
    for row, seed in zip(both, seeds):
        assert [int(v) for v in row] == tr.ranlux48_stream(seed, 40), seed
    assert tr.ranlux48_stream(2147483563, 5) == tr.ranlux48_stream(1, 5)


@pytest.mark.parametrize("Ngrid", [2, 5, 16])
def test_seed_table_matches_restatement(Ngrid):
    for seed in (0, 1, 181171):
        table = sq.thermal_seed_table(seed, Ngrid)
        assert np.array_equal(table, tr.seed_table(seed, Ngrid)), seed
        # the transposed storage: draw number i * Ngrid + j of the stream sits at [i + Ngrid * j]
        stream = tr.ranlux48_stream(seed, Ngrid * Ngrid)
        for i, j in ((0, 1), (1, 0), (Ngrid - 1, 0), (Ngrid - 1, Ngrid - 2)):
            assert int(table[i + Ngrid * j]) == stream[i * Ngrid + j] & 0xFFFFFFFF
    assert not np.array_equal(sq.thermal_seed_table(1, Ngrid).reshape(Ngrid, Ngrid), sq.thermal_seed_table(1, Ngrid).reshape(Ngrid, Ngrid).T)


def _quad_tables(max_fd, min_fd):
    def fd(x):
        return x * x / (math.exp(x) + 1)
    max_fd = min(max_fd, 17.0)
    vel = min_fd + (max_fd - min_fd) * np.arange(tr.NK) / (tr.NK - 1.0)
    pieces = [quad(fd, vel[i], vel[i + 1], epsabs=0, epsrel=1e-13)[0] for i in range(tr.NK - 1)]
    cum = np.array([0.0] + [math.fsum(pieces[:i + 1]) for i in range(tr.NK - 1)])
    total = math.fsum(quad(fd, a, a + 1, epsabs=0, epsrel=1e-13)[0] for a in range(17))
    return vel, cum / cum[-1], cum[-1] / total


@pytest.mark.parametrize("max_fd,min_fd", [(50.0, 0.0), (9.5, 0.25)])
def test_tables_against_quad(max_fd, min_fd):
    vel, cumprob, frac = sq.thermal_tables(max_fd, min_fd)
    qvel, qcum, qfrac = _quad_tables(max_fd, min_fd)
    assert np.array_equal(vel, qvel)
    assert cumprob[0] == 0 and cumprob[-1] == 1 and np.all(np.diff(cumprob) > 0)
    err = np.abs(cumprob[1:] / qcum[1:] - 1).max()
    print(f"max_fd {max_fd} min_fd {min_fd}: cumprob rel err {err:.2e}, total_frac {frac!r} vs {qfrac!r}")
    assert err < 1e-10 and abs(frac / qfrac - 1) < 1e-10
    rvel, rcum, rfrac = tr.fd_tables(max_fd, min_fd)
    assert np.array_equal(vel, rvel) and np.abs(cumprob[1:] / rcum[1:] - 1).max() < 1e-10 and abs(frac / rfrac - 1) < 1e-10


def test_tables_pass_the_reference_gate():
    """libgenic/tests/test_thermal.cpp:29-40: init_thermalvel(100, 5000 / 100, 0)"""
    vel, cumprob, frac = sq.thermal_tables(5000 / 100, 0)
    assert vel[0] == 0 and vel[-1] == 17.0
    half = vel[np.argmax(cumprob >= 0.5)]
    print(f"speed at the first cumprob >= 0.5: {half!r}; total_frac {frac!r}")
    assert abs(half / 2.839075 - 1) < 0.002
    assert abs(frac - 1) < 1e-12          # the whole interval [0, 17]


def test_slopes_against_scipy_makima():
    vel, cumprob, _ = sq.thermal_tables(50.0)
    s = tr.makima_slopes(cumprob, vel)
    ak = Akima1DInterpolator(cumprob, vel, method="makima")
    ref = ak(cumprob, 1)
    assert np.all(np.abs(s - ref) <= 4 * np.spacing(np.abs(ref)))
    p = np.random.default_rng(3).uniform(0, 1, 20000)
    F, ibin = tr.hermite(cumprob, vel, s, p)
    assert np.abs(F - ak(p)).max() < 5e-14
    assert np.all((cumprob[ibin] <= p) & (p < cumprob[ibin + 1]))
    # at the knots the interpolant returns the knot, and the last bin is 1998
    Fk, ik = tr.hermite(cumprob, vel, s, cumprob)
    assert np.array_equal(Fk[:-1], vel[:-1]) and abs(Fk[-1] - vel[-1]) < 1e-14 and ik[-1] == tr.NK - 2 and np.array_equal(ik[:-1], np.arange(tr.NK - 1))
    # a flat stretch has both weights zero: slope 0, not NaN
    assert np.array_equal(tr.makima_slopes(np.arange(6.0), np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])), np.zeros(6))


def test_statistical_gates_of_the_reference():
    """libgenic/tests/test_thermal.cpp:41-64: ranlux48(0), 100 000 particles from one stream, v_amp = 100, max_fd = 50, each added to
    a zero float velocity"""
    vel, cumprob, _ = sq.thermal_tables(5000 / 100, 0)
    n = 100000
    raw = np.array(tr.ranlux48_stream(0, 3 * n), dtype=np.uint64).reshape(n, 3)
    dvel, speed, _ = tr.add_thermal_speeds(100.0, cumprob, vel, tr.makima_slopes(cumprob, vel), raw)
    v = dvel.astype(np.float32)
    v2 = np.sqrt((v * v).sum(axis=1, dtype=np.float32).astype(np.float64))
    expect = 3 * math.pi**4 / 90. / 1.202057 * (7. / 8) / (3 / 4.) * 100
    print(f"mean {v2.mean():.3f} (expected {expect:.3f}), min {v2.min():.3f}, max {v2.max():.3f}")
    assert abs(v2.mean() - expect) < 1
    assert v2.min() > 0
    assert v2.max() < 17.0 * 100
    assert np.abs(v2 / speed - 1).max() < 1e-6         # the direction is a unit vector


def test_symbols_and_bad_arguments_of_the_host_calls():
    for name in ("shq_thermal_seed_table", "shq_thermal_tables", "shq_thermal_speeds", "shq_thermal_phase_ms", "shq_thermal_column_draws"):
        assert hasattr(capi.hip, name), name
    assert C.sizeof(capi.ThermalParams) == 32
    t = np.zeros(4, dtype=np.uint32)
    assert capi.hip.shq_thermal_seed_table(1, 2, None) == ERR_INVALID
    assert capi.hip.shq_thermal_seed_table(1, 0, capi.ptr(t)) == ERR_INVALID
    assert capi.hip.shq_thermal_seed_table(1, 46341, capi.ptr(t)) == ERR_INVALID      # Ngrid^2 no longer fits an int
    assert np.all(t == 0)
    v, c = np.full(tr.NK, 7.0), np.full(tr.NK, 7.0)
    f = C.c_double(7.0)
    for max_fd, min_fd in ((1.0, 1.0), (0.5, 1.0), (np.nan, 0.0), (np.inf, 0.0), (3.0, np.nan), (50.0, 17.0), (50.0, 20.0)):
        assert capi.hip.shq_thermal_tables(max_fd, min_fd, capi.ptr(v), capi.ptr(c), C.byref(f)) == ERR_INVALID, (max_fd, min_fd)
    assert capi.hip.shq_thermal_tables(5.0, 0.0, None, capi.ptr(c), C.byref(f)) == ERR_INVALID
    assert capi.hip.shq_thermal_tables(5.0, 0.0, capi.ptr(v), None, C.byref(f)) == ERR_INVALID
    assert capi.hip.shq_thermal_tables(5.0, 0.0, capi.ptr(v), capi.ptr(c), None) == ERR_INVALID
    assert np.all(v == 7.0) and np.all(c == 7.0) and f.value == 7.0
    assert capi.hip.shq_thermal_tables(5.0, 0.0, capi.ptr(v), capi.ptr(c), C.byref(f)) == 0 and v[-1] == 5.0 and 0 < f.value < 1
