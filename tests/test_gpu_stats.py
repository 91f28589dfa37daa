"""The run logs on the device (csrc/stats.hip) against the restatements of stats_restated.py on its shared cases.

Sums: the per-particle addends are exact IEEE in both codes, so any summation order is within (n - 1) 2^-53 sum |addend| of the exact sum
(the reference's own order under OpenMP is unspecified; test_gpu_startup.py uses the same bound).  EnergyIntComp[0] has one pow per
addend, which on the device may differ from glibc's by an ulp: the project's allowance of 5 x 2^-52 relative for a division and two
multiplications around one pow (test_gpu_startup.py's header).  TemperatureComp[0] is compared with the host engine
(shq_cooling_eval_host) on the restatement's inputs: |d(ne/nh)| <= 2.5e-6 between device and host (test_gpu_cooling.py, HARD) and
|d ln T / d(ne/nh)| <= 4 x 0.76 / 3.28 < 1 give 2.5e-6 sum(Mass T) on top of the summation bound.

Largest deviation of TemperatureComp[0] from the host engine's sum, measured on an MI355X over the cases of
test_temperature_against_the_host_engine (printed per case, not asserted): 1.79 x 2^-52 of the sum (n = 65, sorted by type); 11 of the 16
cases equal the correctly rounded sum of the host engine's addends."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shenqi_amd as sq
from shenqi_amd import capi
import stats_restated as sr
from test_gpu_startup import dev, same_bytes, status_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_INVALID, ERR_NOMEM, ERR_STATE = 1, 3, 4
POW5 = 5 * 2.0 ** -52
HARD = 2.5e-6
ORDERS = ("interleaved", "sorted")
VECTORS = (("MomentumComp", "Momentum"), ("AngMomentumComp", "AngMomentum"), ("CenterOfMassComp", "CenterOfMass"))


@pytest.fixture
def tctx(ctx):
    sq.cooling_set_tables(ctx, sr.device_tables())
    return ctx


def sum_bound(addends):
    return max(len(addends) - 1, 0) * 2.0 ** -53 * math.fsum(abs(x) for x in addends)


def run(ctx, k, params, capacity=None):
    L = sq.stats_layout(sph_dtype=k.S.dtype)
    dP, dS = dev(k.P), dev(k.S)
    sums, deferred = sq.energy_statistics(ctx, L, dP, k.n, dS, len(k.S), params, capacity)
    assert same_bytes(dP, k.P) and same_bytes(dS, k.S)
    return sums, deferred


def sums_bytes(s):
    return bytes(s)[:capi.StatsSums.kernel_ms.offset]


def check_plain_sums(s, a, tag):
    """every sum but TemperatureComp against the addends"""
    assert list(s.count) == a["count"] and s.n_bad_type == a["n_bad_type"], tag
    for t in range(6):
        cols = a["by_type"][t]
        got = dict(Mass=s.MassComp[t], EnergyPot=s.EnergyPotComp[t], EnergyKin=s.EnergyKinComp[t])
        for name, stem in VECTORS:
            for j in range(3):
                got["%s%d" % (stem, j)] = getattr(s, name)[t][j]
            assert getattr(s, name)[t][3] == 0, (tag, name, t)
        for c in sr.COLUMNS:
            assert abs(got[c] - math.fsum(cols[c])) <= sum_bound(cols[c]), (tag, t, c, got[c], math.fsum(cols[c]))
        if t > 0:
            assert s.EnergyIntComp[t] == 0 and s.TemperatureComp[t] == 0, (tag, t)
    e = a["eint"]
    assert abs(s.EnergyIntComp[0] - math.fsum(e)) <= sum_bound(e) + POW5 * math.fsum(abs(x) for x in e), (tag, s.EnergyIntComp[0], math.fsum(e))


@pytest.mark.parametrize("n", sr.COUNTS)
def test_sums_without_temperatures(ctx, n):
    """want_temperature = 0 needs no tables (a context that never had any) and leaves TemperatureComp zero"""
    with sq.Context(0) as fresh:
        for order in ORDERS:
            k = sr.case(n, order)
            s, deferred = run(fresh, k, sr.stats_params(capi.COOL_UVBG_GLOBAL, False))
            check_plain_sums(s, sr.energy_addends(k.P, k.S, sr.TIME), (n, order))
            assert not any(s.TemperatureComp) and not any(s.n_status) and s.n_deferred == 0 and len(deferred) == 0
            again = run(fresh, k, sr.stats_params(capi.COOL_UVBG_GLOBAL, False))[0]
            assert sums_bytes(again) == sums_bytes(s), (n, order)


def test_a_type_above_five_is_counted_and_adds_nothing(ctx):
    k = sr.case(257, "interleaved", True)
    a = sr.energy_addends(k.P, k.S, sr.TIME)
    assert a["n_bad_type"] == 1 and sum(a["count"]) == 256
    s, _ = run(ctx, k, sr.stats_params(capi.COOL_UVBG_GLOBAL, False))
    check_plain_sums(s, a, "type 6")


CASES = [(n, order, capi.COOL_UVBG_GLOBAL) for n in sr.COUNTS for order in ORDERS] + [(257, "interleaved", capi.COOL_UVBG_ZREION), (257, "sorted", capi.COOL_UVBG_J21)]


@pytest.mark.parametrize("n,order,mode", CASES)
def test_temperature_against_the_host_engine(tctx, n, order, mode):
    k = sr.case(n, order)
    a = sr.energy_addends(k.P, k.S, sr.TIME)
    T, status = sr.temperatures(n, order, mode)
    s, deferred = run(tctx, k, sr.stats_params(mode))
    tag = (n, order, mode)
    check_plain_sums(s, a, tag)
    ok = status == capi.COOL_OK
    addends = [float(x) for x in a["mass"][ok] * T[ok]]
    want = math.fsum(addends)
    dev_ulps = abs(s.TemperatureComp[0] - want) / (2.0 ** -52 * want) if want > 0 else 0.0
    print("TemperatureComp[0] n=%d %s mode %d: %d solves, %d not OK, deviation %.3g x 2^-52" % (n, order, mode, len(T), int((~ok).sum()), dev_ulps))
    assert abs(s.TemperatureComp[0] - want) <= sum_bound(addends) + HARD * want, (tag, s.TemperatureComp[0], want)
    assert list(s.n_status) == [int((status == q).sum()) for q in range(4)], tag
    assert np.array_equal(deferred, a["gas"][~ok]) and s.n_deferred == int((~ok).sum()), tag
    again, deferred2 = run(tctx, k, sr.stats_params(mode))
    assert sums_bytes(again) == sums_bytes(s) and np.array_equal(deferred2, deferred), tag


def test_a_deferred_list_one_short(tctx):
    k = sr.case(1000)
    full, deferred = run(tctx, k, sr.stats_params(capi.COOL_UVBG_GLOBAL))
    assert len(deferred) >= 2
    L = sq.stats_layout(sph_dtype=k.S.dtype)
    with pytest.raises(capi.ShqError, match="status 3") as e:
        sq.energy_statistics(tctx, L, dev(k.P), k.n, dev(k.S), len(k.S), sr.stats_params(capi.COOL_UVBG_GLOBAL), len(deferred) - 1)
    assert sums_bytes(e.value.sums) == sums_bytes(full) and e.value.sums.n_deferred == len(deferred)
    assert np.array_equal(e.value.deferred, deferred[:-1])


def untouched_call(ctx, k, L, params, dP=None, dS=None, nsph=None):
    """the status of a refused call; the outputs keep their pattern"""
    sums = capi.StatsSums()
    C.memset(C.byref(sums), 0x5A, C.sizeof(sums))
    before = bytes(sums)
    deferred = np.full(8, -7, dtype=np.int32)
    dP = dev(k.P) if dP is None else dP
    dS = dev(k.S) if dS is None else dS
    rc = capi.hip.shq_energy_statistics(ctx.h, C.byref(L), dP.data_ptr(), k.n, dS.data_ptr(), len(k.S) if nsph is None else nsph, C.byref(params), C.byref(sums),
                                        capi.ptr(deferred), len(deferred))
    assert bytes(sums) == before and np.all(deferred == -7)
    return rc


def test_state_errors(ctx):
    k = sr.case(257)
    L = sq.stats_layout(sph_dtype=k.S.dtype)
    with sq.Context(0) as fresh:        # a context that never had tables
        assert untouched_call(fresh, k, L, sr.stats_params(capi.COOL_UVBG_GLOBAL)) == ERR_STATE
        sq.cooling_set_tables(fresh, sr.cooling().tables())      # no Zreion table
        assert untouched_call(fresh, k, L, sr.stats_params(capi.COOL_UVBG_ZREION)) == ERR_STATE


def test_invalid_arguments(tctx):
    k = sr.case(257)
    L = sq.stats_layout(sph_dtype=k.S.dtype)
    par = sr.stats_params(capi.COOL_UVBG_GLOBAL)
    gas = np.flatnonzero(k.P["Type"] == 0)
    for bad in (-1, len(k.S)):          # a gas PI outside [0, nsph)
        P = k.P.copy()
        P["PI"][gas[-1]] = bad
        dP = dev(P)
        assert untouched_call(tctx, k, L, par, dP=dP) == ERR_INVALID
        assert untouched_call(tctx, k, L, sr.stats_params(capi.COOL_UVBG_GLOBAL, False), dP=dP) == ERR_INVALID
        assert same_bytes(dP, P)
    # another type's PI is not looked at
    P = k.P.copy()
    P["PI"][np.flatnonzero(k.P["Type"] == 1)] = -5
    sq.energy_statistics(tctx, L, dev(P), k.n, dev(k.S), len(k.S), par)
    # J21 mode with either field missing
    for member in ("sph_off_local_j21", "sph_off_zreion"):
        Lj = sq.stats_layout(sph_dtype=k.S.dtype)
        setattr(Lj, member, capi.NOFIELD)
        assert untouched_call(tctx, k, Lj, sr.stats_params(capi.COOL_UVBG_J21)) == ERR_INVALID
        sq.energy_statistics(tctx, Lj, dev(k.P), k.n, dev(k.S), len(k.S), par)      # the other modes do not need them
    # the layout rules of the record pass
    for member, value in (("part_elsize", 164), ("part_elsize", 248), ("off_pos", 4), ("off_pos", 144), ("off_mass", 30), ("off_type", 160), ("off_pi", 34),
                          ("off_vel", 140), ("off_potential", 156), ("off_potential", capi.NOFIELD), ("sph_elsize", 204), ("sph_off_density", 196),
                          ("sph_off_entropy", 20), ("sph_off_ne", 200)):
        Lb = sq.stats_layout(sph_dtype=k.S.dtype)
        setattr(Lb, member, value)
        assert untouched_call(tctx, k, Lb, par) == ERR_INVALID, (member, value)
    dP = dev(k.P)
    rc = capi.hip.shq_energy_statistics(tctx.h, C.byref(L), dP.data_ptr() + 4, k.n - 1, dev(k.S).data_ptr(), len(k.S), C.byref(par),
                                        C.byref(capi.StatsSums()), None, 0)
    assert rc == ERR_INVALID            # a misaligned record array


# ---- black holes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (0, 1, 65, 1000))
def test_bh_totals(ctx, n):
    B = sr.bh_slots(n)
    num, addends = sr.bh_totals(B)
    assert n < 3 or 0 < num < n
    dB = dev(B)
    got_num, got = sq.bh_totals(ctx, dB, n)
    assert got_num == num
    for c in range(3):
        assert abs(got[c] - math.fsum(addends[c])) <= sum_bound(addends[c]), (n, c, got[c], math.fsum(addends[c]))
    again = sq.bh_totals(ctx, dB, n)
    assert again[0] == num and again[1].tobytes() == got.tobytes() and same_bytes(dB, B)


def dev_arrays(priv, names=None):
    return {k: torch.from_numpy(np.array(v.view(np.int64) if v.dtype == np.uint64 else v)).to(DEV) for k, v in priv.items() if names is None or k in names}


def details(ctx, k, arrays, active, P=None, n_swallow=None, spare=2):
    """the call on a pattern-filled output with `spare` records of room behind the last; (records, bytes behind them)"""
    L = sq.bh_detail_layout()
    X = sq.bh_detail_arrays(arrays, len(k.priv["SPH_SwallowID"]) if n_swallow is None else n_swallow, sr.OFFSET)
    m = len(active)
    out = torch.full(((m + spare) * capi.BHINFO_SIZE,), 0xA5, dtype=torch.uint8, device=DEV)
    dA = torch.from_numpy(np.ascontiguousarray(active, dtype=np.int32)).to(DEV) if m else None
    P = k.P if P is None else P
    dP, dB = dev(P), dev(k.B)
    info = sq.bh_details(ctx, L, dP, len(P), dB, len(k.B), X, dA, m, 0.3125, d_out=out)
    assert same_bytes(dP, P) and same_bytes(dB, k.B)
    return info, out.cpu().numpy()[m * capi.BHINFO_SIZE:]


@pytest.mark.parametrize("m", (0, 1, 65, 300))
def test_bh_details_equal_the_restatement(ctx, m):
    k = sr.bh_case()
    active = k.active(m)
    assert m < 2 or np.any(np.diff(active) < 0)
    want = sr.bh_info(k.P, k.B, k.priv, active, 0.3125, sr.OFFSET)
    info, behind = details(ctx, k, dev_arrays(k.priv), active)
    assert info.tobytes() == want.tobytes()
    assert np.all(behind == 0xA5) and len(behind) == 2 * capi.BHINFO_SIZE


def test_bh_details_of_the_first_particles_without_a_list(ctx):
    k = sr.bh_case()
    P = k.P.copy()
    first = k.P[k.bh[:7]]
    P[:7] = first
    L = sq.bh_detail_layout()
    X = sq.bh_detail_arrays(dev_arrays(k.priv), len(k.priv["SPH_SwallowID"]), sr.OFFSET)
    info = sq.bh_details(ctx, L, dev(P), len(P), dev(k.B), len(k.B), X, None, 7, 0.3125)
    assert info.tobytes() == sr.bh_info(P, k.B, k.priv, np.arange(7), 0.3125, sr.OFFSET).tobytes()


@pytest.mark.parametrize("missing", capi.BH_DETAIL_ARRAYS)
def test_bh_details_with_a_null_array(ctx, missing):
    k = sr.bh_case()
    active = k.active(65)
    priv = {name: v for name, v in k.priv.items() if name != missing}
    want = sr.bh_info(k.P, k.B, priv, active, 0.3125, sr.OFFSET)
    assert not want[missing].any()
    info, behind = details(ctx, k, dev_arrays(priv), active)
    assert info.tobytes() == want.tobytes() and np.all(behind == 0xA5)


def test_bh_details_invalid(ctx):
    k = sr.bh_case()
    active = k.active(65)
    arrays = dev_arrays(k.priv)
    for bad in (-1, len(k.P)):          # an active index outside [0, numpart): the reference's test lets numpart through
        act = active.copy()
        act[40] = bad
        assert status_of(lambda: details(ctx, k, arrays, act)) == ERR_INVALID
    act = active.copy()
    act[3] = np.flatnonzero(k.P["Type"] != 5)[10]       # "Supposed BH ... has type ..."
    assert status_of(lambda: details(ctx, k, arrays, act)) == ERR_INVALID
    for bad in (-1, len(k.B)):          # a PI outside the slots
        P = k.P.copy()
        P["PI"][active[64]] = bad
        assert status_of(lambda: details(ctx, k, arrays, active, P=P)) == ERR_INVALID
    # a PI inside the slots and outside SPH_SwallowID; fine without that array
    pi_max = int(k.P["PI"][active].max())
    assert status_of(lambda: details(ctx, k, arrays, active, n_swallow=pi_max)) == ERR_INVALID
    assert status_of(lambda: details(ctx, k, {n: v for n, v in arrays.items() if n != "SPH_SwallowID"}, active, n_swallow=0)) == 0
    assert status_of(lambda: details(ctx, k, arrays, active, n_swallow=pi_max + 1)) == 0
