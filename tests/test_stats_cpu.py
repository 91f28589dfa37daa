"""The host side of the run logs (csrc/stats.hip, shenqi_amd/stats.py): shq_stats_finish against the restatement byte for byte, the three
log lines against libc's snprintf with the reference's format strings, the BHinfo layout.  No GPU."""
import ctypes as C
import ctypes.util
import math

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import stats_restated as sr

ERR_INVALID = 1
libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")

ENERGY_FMT = b"%g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g\n"     # stats.cpp:384
BLACKHOLES_FMT = b"%g %d %g %g %g %g\n"                                                                    # bhinfo.cpp:199
SFR_FMT = b"%.12g %g %g %g %g %g %ld %ld\n"                                                                # sfr_eff.cpp:415


def c_line(fmt, *args):
    buf = C.create_string_buffer(4096)
    n = libc.snprintf(buf, C.c_size_t(len(buf)), fmt, *args)
    assert 0 < n < len(buf)
    return buf.value.decode()


def random_sums(seed, special=False):
    rng = np.random.default_rng([sr.SEED, seed])
    s = capi.StatsSums()
    d = {}
    for name in ("MassComp", "EnergyPotComp", "EnergyKinComp", "EnergyIntComp", "TemperatureComp"):
        v = rng.normal(size=6) * 10.0 ** rng.uniform(-3, 8, 6)
        if name == "MassComp":
            v = np.abs(v)
            v[3] = 0.0                       # a type without particles: no division
            if special:
                v[4] = -v[4]                 # a negative mass sum is not divided by either
        if special and name != "MassComp":
            v[1], v[2], v[5] = 0.0, 1e-300, -1e-300
        d[name] = [float(x) for x in v]
        for i in range(6):
            getattr(s, name)[i] = d[name][i]
    for name in ("MomentumComp", "AngMomentumComp", "CenterOfMassComp"):
        v = rng.normal(size=(6, 4)) * 10.0 ** rng.uniform(-3, 8, (6, 4))
        v[:, 3] = 0.0
        if special:
            v[2] = 0.0
            v[5, 1] = 1e-300
        d[name] = [[float(x) for x in r] for r in v]
        for i in range(6):
            for j in range(4):
                getattr(s, name)[i][j] = d[name][i][j]
    return s, d


def same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("seed,special", [(0, False), (1, False), (2, True), (3, True)])
def test_stats_finish_equals_the_restatement_byte_for_byte(seed, special):
    s, d = random_sums(seed, special)
    got, want = sq.stats_finish(s), sr.finish(d)
    for k in ("Mass", "EnergyKin", "EnergyPot", "EnergyInt", "EnergyTot"):
        assert same(getattr(got, k), want[k]), k
    for k in ("Momentum", "AngMomentum", "CenterOfMass"):
        for j in range(4):
            assert same(getattr(got, k)[j], want[k][j]), (k, j)
    for k in ("MassComp", "EnergyKinComp", "EnergyPotComp", "EnergyIntComp", "EnergyTotComp", "TemperatureComp"):
        for i in range(6):
            assert same(getattr(got, k)[i], want[k][i]), (k, i)
    for k in ("MomentumComp", "AngMomentumComp", "CenterOfMassComp"):
        for i in range(6):
            for j in range(4):
                assert same(getattr(got, k)[i][j], want[k][i][j]), (k, i, j)
    assert got.TemperatureComp[3] == s.TemperatureComp[3] and got.CenterOfMassComp[3][0] == s.CenterOfMassComp[3][0]


def energy_args(Time, s):
    a = [Time, s.TemperatureComp[0], s.EnergyInt, s.EnergyPot, s.EnergyKin]
    for t in range(6):
        a += [s.EnergyIntComp[t], s.EnergyPotComp[t], s.EnergyKinComp[t]]
    return a + [s.MassComp[t] for t in range(6)]


@pytest.mark.parametrize("seed,special", [(0, False), (2, True), (3, True)])
def test_energy_line_equals_snprintf(seed, special):
    state = sq.stats_finish(random_sums(seed, special)[0])
    for Time in (0.25, 1.0, 0.0123456789, 1e-300):
        want = c_line(ENERGY_FMT, *[C.c_double(x) for x in energy_args(Time, state)])
        assert sq.energy_line(Time, state) == want
    assert len(sq.energy_line(0.25, state).split()) == 29


def test_energy_line_of_an_empty_rank():
    state = sq.stats_finish(capi.StatsSums())
    assert sq.energy_line(0.5, state) == "0.5" + " 0" * 28 + "\n"


UNITS = dict(UnitMass_in_g=1.989e43, UnitTime_in_s=3.08568e16)


def blackholes_args(atime, num, sums, units):
    total_mass_holes, total_mdot, total_mdoteddington = sums
    mdot_in_msun_per_year = total_mdot * (units["UnitMass_in_g"] / 1.989e33) / (units["UnitTime_in_s"] / 3.155e7)
    total_mdoteddington *= 1.0 / ((4 * math.pi * 6.672e-8 * 2.99792458e10 * 1.6726e-24 / (0.1 * 2.99792458e10 * 2.99792458e10 * 6.65245e-25)) * units["UnitTime_in_s"])
    return [C.c_double(atime), C.c_int(num), C.c_double(total_mass_holes), C.c_double(total_mdot), C.c_double(mdot_in_msun_per_year), C.c_double(total_mdoteddington)]


@pytest.mark.parametrize("num,sums", [(0, (0.0, 0.0, 0.0)), (3, (1.25e-3, 4.5e-7, 3.3e-4)), (123456, (-7.0, 1e-300, -1e-300)), (1, (1e300, 12345678.9, 0.1))])
def test_blackholes_line_equals_snprintf(num, sums):
    for atime in (0.1, 0.3333333333, 1.0):
        assert sq.blackholes_line(atime, num, sums, UNITS) == c_line(BLACKHOLES_FMT, *blackholes_args(atime, num, sums, UNITS))

    class U:
        UnitMass_in_g, UnitTime_in_s = UNITS["UnitMass_in_g"], UNITS["UnitTime_in_s"]
    assert sq.blackholes_line(0.1, num, sums, U) == sq.blackholes_line(0.1, num, sums, UNITS)


def sfr_args(Time, sums, counts, unit):
    total_sm, totsfrrate, total_sum_mass_stars, total_sum_dtime = sums
    total_sum_part, tot_new = counts
    rate = 0.0
    if total_sum_dtime > 0:
        rate = total_sm * total_sum_part / total_sum_dtime
    with np.errstate(all="ignore"):
        mean = float(np.float64(total_sum_dtime) / np.float64(total_sum_part))
    return [C.c_double(Time), C.c_double(total_sm), C.c_double(totsfrrate), C.c_double(rate * unit), C.c_double(total_sum_mass_stars), C.c_double(mean),
            C.c_long(total_sum_part), C.c_long(tot_new)]


@pytest.mark.parametrize("sums,counts", [((2.5e-3, 0.75, 2.0e-3, 3.0e-4), (17, 2)), ((1e-300, -0.5, 0.0, 1e-300), (1, 0)), ((4.0, 1e5, 3.9, 0.0), (12, 12)),
                                         ((1.0, 2.0, 3.0, 4.0), (5000000000, 3))])
def test_sfr_line_equals_snprintf(sums, counts):
    unit = 1.022e1
    for Time in (0.25, 0.123456789012345, 1.0):
        assert sq.sfr_line(Time, sums, counts, unit) == c_line(SFR_FMT, *sfr_args(Time, sums, counts, unit))


def test_sfr_line_without_stars_and_without_time():
    assert sq.sfr_line(0.25, (0.0, 1.0, 0.0, 1.0), (3, 0), 10.0) is None
    assert sq.sfr_line(0.25, (-1.0, 1.0, 0.0, 1.0), (3, 0), 10.0) is None
    line = sq.sfr_line(0.25, (2.0, 1.0, 0.5, 0.0), (3, 1), 10.0)            # total_sum_dtime == 0: rate = 0
    assert line.split()[3] == "0" and line == "0.25 2 1 0 0.5 0 3 1\n"


def test_bhinfo_dtype_is_the_packed_struct():
    d = sq.BHINFO_DTYPE
    assert d.itemsize == 436 == capi.BHINFO_SIZE
    want = dict(size1=0, ID=4, Mass=12, Mdot=20, Density=28, minTimeBin=36, encounter=40, MinPotPos=44, MinPot=68, BH_Entropy=76, BH_SurroundingGasVel=84,
                BH_accreted_momentum=108, BH_accreted_Mass=132, BH_accreted_BHMass=140, BH_FeedbackWeightSum=148, SPH_SwallowID=156, SwallowID=164,
                CountProgs=172, Swallowed=176, Pos=180, BH_SurroundingDensity=204, BH_SurroundingParticles=212, BH_SurroundingVel=220,
                BH_SurroundingRmsVel=244, BH_DFAccel=252, BH_DragAccel=276, BH_FullTreeGravAccel=300, Velocity=324, Mtrack=348, Mdyn=356,
                KineticFdbkEnergy=364, NumDM=372, V1sumDM=380, VDisp=404, MgasEnc=412, KEflag=420, a=424, size2=432)
    assert {k: d.fields[k][1] for k in d.names} == want
    # the members are packed: each begins where the one before it ends
    end = 0
    for k in d.names:
        assert d.fields[k][1] == end, k
        end += d.fields[k][0].itemsize
    assert end == 436


def test_the_restated_bh_records():
    """the restatement itself: sizes, the zero members, the offset"""
    k = sr.bh_case()
    act = k.active(5)
    info = sr.bh_info(k.P, k.B, k.priv, act, 0.5, sr.OFFSET)
    assert np.all(info["size1"] == 428) and np.all(info["size2"] == 428) and not info["V1sumDM"].any() and not info["BH_SurroundingParticles"].any()
    assert np.array_equal(info["Pos"], k.P["Pos"][act] - np.array(sr.OFFSET)) and np.array_equal(info["ID"], k.P["ID"][act])
    bare = sr.bh_info(k.P, k.B, {}, act, 0.5, sr.OFFSET)
    assert not bare["BH_Entropy"].any() and not bare["SPH_SwallowID"].any() and np.array_equal(bare["Mass"], info["Mass"])


def test_argument_errors():
    state = capi.StatsState()
    assert capi.hip.shq_stats_finish(None, C.byref(state)) == ERR_INVALID
    assert capi.hip.shq_stats_finish(C.byref(capi.StatsSums()), None) == ERR_INVALID
    with pytest.raises(ValueError):
        sq.bh_detail_arrays({"BH_Entropi": None})
    with pytest.raises(KeyError):
        sq.blackholes_line(0.5, 1, (1.0, 1.0, 1.0), dict(UnitMass_in_g=1.0))
    with pytest.raises(ValueError):
        sq.sfr_line(0.5, (1.0, 1.0, 1.0), (1, 1), 1.0)           # four sums
    L = sq.stats_layout(sph_dtype=sr.SPH_DTYPE)
    assert L.part_elsize == 160 and L.sph_off_local_j21 == 176 and sq.stats_layout().sph_off_zreion == capi.NOFIELD
