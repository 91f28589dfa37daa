"""Star formation on the device (shq_sfr_eval, shq_sfr_on_eeqos, shq_starformation; csrc/sfr.hip driving csrc/sfr_math.hpp) against the
same engine on the host (shq_sfr_eval_host, which test_sfr_cpu.py holds bit-equal to the Python restatement of sfr_eff.cpp).  Every test
restores what it changes on the shared context.  The spawn chain behind the lists (shq_slots_split_particles, shq_make_particle_stars)
works on opaque device records and is shown in INTEGRATION.md; it has its own tests in test_gpu_exchange.py."""
import functools

import numpy as np
import pytest

import shenqi_amd as sq
from shenqi_amd import capi
import cooling_restated as cr
import sfr_cases as sc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# ---- Device against host engine, the dense set with its edge rows (sfr_cases.particles, seed 20261018, 2089 particles) ----------------
# Discrete outputs (status, decision, flag byte, branch byte, and whether a cooling time is zero) must be equal for EVERY particle: the
# seed was chosen so that a host build whose every libm result is off by one ulp flips none of them (test_sfr_cpu.py recomputes that),
# and the card's libm is closer to glibc's than that build.
#
# Hard bounds, derived.  The starting figures are the project's device-to-host ones (test_gpu_cooling.py): ne within HARD = 2.5e-6 of
# the host's (the fixed point's ITERCONV is 1e-6, whatever the starting guess), and one GetCoolingTime within T = 10 * HARD relative.
# Everything else a particle computes before a cooling time enters (tsfr, factorEVP, egyhot, the H2 and self-gravity factors, enttou) is
# a handful of libm calls on identical inputs, i.e. a few 2^-52 relative; R = 1e-9 stands for all of that and for the rounding of the
# operations below, see (*).
#   y         = tsfr / tcool * egyhot / const                    rel  T
#   cloudfrac = x(y), the root of x / (1 - x)^2 = y:  dx / x = (1 - x) / (1 + x) dy / y, so the condition number is <= 1:  rel  T
#               and d(1 - x) / (1 - x) = -x / (1 + x) dy / y:  rel  T / 2
#   trelax    = tsfr (1 - x) / x / const:  rel  T / 2 + T = 1.5 T
#   smr, sm   = const cloudfrac Mass / tsfr (x factors of the inputs):  rel  T
#   dM, Sfr, prob: Mass (1 - e^-p) with p = sm / Mass:  d(1 - e^-p) / (1 - e^-p) = [p e^-p / (1 - e^-p)] dp / p, bracket <= 1:  rel  T
#   Metallicity = Z + w 0.02 (1 - e^-p) / Generations (x (1 - w) more):  abs  0.02 T
#   Ne        : abs  HARD
#   egyeff    = cold x + (1 - x) egyhot:  abs  egyhot x T  <= egyeff-scale T
#   Entropy densityfac = egyeff + (egycurrent - egyeff) e^-q,  q = dtime / trelax, trelax from the line above or a second cooling time:
#               d = d(egyeff) (1 - e^-q) + (egycurrent - egyeff) (q e^-q) d(trelax) / trelax,  |q e^-q| <= 1 / e:
#               abs  [T + 1.5 T / e] max(egycurrent, egyeff)  <=  2 T max(egycurrent, egyeff)
# (*) x(y) is computed as 1 + s - sqrt(2 s + s^2) with s = 1 / (2 y), which cancels for small y: each side carries a rounding error of
# a few 2^-52 (1 + s), i.e. 16 * 2^-52 (1 + s) / x relative between the two; the test asserts on the host's values that this is below R.
# The relative rows get 1.5 T + R, which is the largest of the figures above.
HARD = 2.5e-6
T = 10 * HARD
R = 1e-9
REL_ROWS = ("trelax", "tsfr", "egyhot", "cloudfrac", "smr", "sm", "dM", "Sfr", "mass_of_star", "prob", "egyeff4", "tcool_relax", "egyeff", "egycurrent", "trelax_used")
REL_BOUND = 1.5 * T + R
# Tight bounds, measured on an MI355X: the largest deviation once the 0.1 % largest are set aside, in units of 2^-52 (relative for the
# rows above, absolute for Ne, and for Entropy in units of 2^-52 max(egycurrent, egyeff) / densityfac).  The bound is 8 x the measured
# value, as in test_gpu_cooling.py and for its reason: the card's libm differs from glibc's in the last bits only.
# Measured (the largest of the four BHFeedbackUseTcool runs; all 2089 particles agree in every discrete outcome and in the step counts):
#   relative rows 25.66 outside the 0.1 % (497 at most: cloudfrac's cancellation at small y carries a cooling time's last bits far),
#   Ne 1 (3 at most), Metallicity 0.0156 (0.031 at most), Entropy 1.73 (2.28 at most).
TIGHT_MEASURED = {"rel": 25.66, "Ne": 1.0, "Metallicity": 0.01562, "Entropy": 1.732}
OUTLIER_SHARE = 1e-3


def _restore(ctx):
    capi.check(capi.hip.shq_set_inputs_current(ctx.h, 0))
    sq.cooling_set_refill(ctx, 1)
    sq.sfr_set_refill(ctx, 1)


@pytest.fixture
def sctx(ctx):
    _restore(ctx)
    sq.cooling_set_tables(ctx, sc.case().tables())
    try:
        yield ctx
    finally:
        _restore(ctx)


def _eval(ctx, what, par, p, local_uv=None):
    c = sc.case()
    return sq.sfr_eval(ctx, sc.lib_params(par), what, p, c.uvbg(), sc.REDSHIFT, sc.A3INV, sc.HUBBLE, sc.rnd_table(),
                       uvbg_local=None if local_uv is None else c.uvbg(local_uv))


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a.arrays(), b.arrays()))


def _outside_share(d):
    keep = len(d) - int(np.floor(OUTLIER_SHARE * len(d)))
    return float(np.sort(d)[keep - 1])


def _deviations(dev, host, p):
    """per group, in units of 2^-52, over the particles (of the inputs p) that are OK on both sides"""
    ok = (host.status == capi.COOL_OK) & (dev.status == capi.COOL_OK)
    rel = np.zeros(ok.sum())
    with np.errstate(all="ignore"):
        for name in REL_ROWS:
            h, d = getattr(host, name)[ok], getattr(dev, name)[ok]
            rel = np.maximum(rel, np.where(h == d, 0.0, np.abs(d - h) / np.abs(h)))
        densityfac = host.egycurrent[ok] / np.asarray(p["Entropy"])[ok]
        scale = np.maximum(host.egycurrent[ok], host.egyeff[ok]) / densityfac
        ent = np.where(host.branch[ok] & capi.SFR_B_RELAXED, np.abs(dev.Entropy[ok] - host.Entropy[ok]) / scale, np.abs(dev.Entropy[ok] - host.Entropy[ok]))
    return {"rel": rel / EPS, "Ne": np.abs(dev.Ne[ok] - host.Ne[ok]) / EPS, "Metallicity": np.abs(dev.Metallicity[ok] - host.Metallicity[ok]) / EPS, "Entropy": ent / EPS}


# ---- (1) launch shapes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 65, 2048 + 37])
def test_launch_shapes(sctx, n):
    """less than a wave, a wave and one lane, and 2085: two workgroups' shares with a ragged end, every lane refilled"""
    par, p = sc.params(), sc.subset(sc.particles(), slice(0, n))
    a = _eval(sctx, "STARFORM", par, p)
    b = _eval(sctx, "STARFORM", par, p)
    sq.sfr_set_refill(sctx, 0)
    c = _eval(sctx, "STARFORM", par, p)
    assert _same(a, b)      # two runs
    assert _same(a, c)      # refill on and off
    host = sc.host_starform()
    assert np.array_equal(a.status, host.status[:n]) and np.array_equal(a.decision, host.decision[:n]) and np.array_equal(a.branch, host.branch[:n])
    ms, steps = sq.sfr_last_kernel(sctx)
    assert ms > 0 and steps == int(c.steps.sum()) and steps > 0


# ---- (2) device against the host engine -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tcool", [0, 1, 2, 3])
def test_device_against_host_engine(sctx, tcool):
    p = sc.particles()
    dev = _eval(sctx, "STARFORM", sc.params(BHFeedbackUseTcool=tcool), p)
    host = sc.host_starform(tcool)
    dv = _deviations(dev, host, p)
    print(f"sfr device vs host, BHFeedbackUseTcool {tcool}: " + "; ".join(f"{k} outside the share {_outside_share(v):.4g}, max {v.max():.4g}" for k, v in dv.items()) +
          f"; steps equal {np.mean(dev.steps == host.steps):.5f}")
    # discrete, every particle
    assert np.array_equal(dev.status, host.status)
    assert np.array_equal(dev.decision, host.decision) and np.array_equal(dev.flags, host.flags) and np.array_equal(dev.branch, host.branch)
    ok = host.status == capi.COOL_OK
    assert np.array_equal(dev.tcool_relax[ok] == 0, host.tcool_relax[ok] == 0) and np.array_equal(dev.trelax[ok] == 0, host.trelax[ok] == 0)
    assert np.array_equal(dev.egycold[ok], host.egycold[ok]) and np.array_equal(dev.ne_eeqos[ok], dev.Ne[ok])
    # (*) of the derivation
    x = host.cloudfrac[ok][(host.cloudfrac[ok] > 0) & (host.cloudfrac[ok] < 1)]
    assert np.all(16 * EPS * (1 + (1 - x) ** 2 / (2 * x)) / x < R)
    # hard
    assert np.all(dv["rel"] * EPS <= REL_BOUND), np.flatnonzero(dv["rel"] * EPS > REL_BOUND)[:5]
    assert np.all(dv["Ne"] * EPS <= HARD) and np.all(dv["Metallicity"] * EPS <= 0.02 * T)
    assert np.all(dv["Entropy"] * EPS <= 2 * T)
    # tight
    for k, v in dv.items():
        assert np.mean(v > 8 * TIGHT_MEASURED[k]) <= OUTLIER_SHARE, k


@pytest.mark.parametrize("tcool", [0, 1, 3])
def test_net_heating_against_host_engine(sctx, tcool):
    """the synthetic strong-heating UVBG as the local one, on the first 256 particles and the edge rows: GetCoolingTime returns 0, and the
    unguarded IEEE path (tsfr / 0 = inf, cloudfrac = 1, trelax = 0, exp(-dtime / 0) = 0, a zero cooling time in cooling_relaxed) runs with
    the card's division, sqrt and exp"""
    uv, p, par = sc.heating_uvbg(), sc.heating_subset(), sc.params(BHFeedbackUseTcool=tcool)
    dev, host = _eval(sctx, "STARFORM", par, p, local_uv=uv), sc.host("STARFORM", par, p, local_uv=uv)
    assert np.array_equal(dev.status, host.status) and np.array_equal(dev.steps, host.steps)
    ok = host.status == capi.COOL_OK
    for k in ("decision", "flags", "branch"):
        assert np.array_equal(getattr(dev, k)[ok], getattr(host, k)[ok]), k
    on = ok & ((host.branch & capi.SFR_B_ON_EEQOS) != 0)
    assert on.sum() > 200 and np.all(dev.cloudfrac[on] == 1) and np.all(dev.trelax[on] == 0) and np.all(dev.trelax_used[on] == 0)
    assert np.all(dev.tcool_relax[ok] == 0) and np.all(host.tcool_relax[ok] == 0)
    if tcool:
        assert ((host.branch[on] & capi.SFR_B_TCOOL) != 0).sum() > 20 and not (host.branch[on] & capi.SFR_B_TCOOL_WON).any()
    rel = on & ((host.branch & capi.SFR_B_RELAXED) != 0)
    assert rel.sum() > 100 and np.all(dev.egyeff[rel] == par["EgySpecCold"])        # the relaxation lands on egyeff = EgySpecCold at once
    dv = _deviations(dev, host, p)
    assert np.all(dv["rel"] * EPS <= REL_BOUND) and np.all(dv["Ne"] * EPS <= HARD) and np.all(dv["Metallicity"] * EPS <= 0.02 * T) and np.all(dv["Entropy"] * EPS <= 2 * T)
    for k, v in dv.items():
        assert np.mean(v > 8 * TIGHT_MEASURED[k]) <= OUTLIER_SHARE, k
    nh = _eval(sctx, "NH0", sc.params(), p, local_uv=uv), sc.host("NH0", sc.params(), p, local_uv=uv)
    k0 = nh[1].status == capi.COOL_OK
    assert np.array_equal(nh[0].status, nh[1].status) and np.all(np.abs(nh[0].query[k0] - nh[1].query[k0]) <= (2 * T + R) * np.abs(nh[1].query[k0]))


@pytest.mark.parametrize("what", ["EGYEFF", "NH0", "HE0", "HEP", "HEPP", "ON_EEQOS"])
def test_queries_against_host_engine(sctx, what):
    """the other modes on the first 300 particles and the edge rows, under BHFeedbackUseTcool == 2 so that the fourth clause runs"""
    par = sc.params(BHFeedbackUseTcool=2)
    n = len(sc.particles()["Density"])
    p = sc.subset(sc.particles(), np.r_[0:300, n - len(sc.EDGE_ROWS):n])
    dev, host = _eval(sctx, what, par, p), sc.host(what, par, p)
    ok = host.status == capi.COOL_OK
    assert np.array_equal(dev.status, host.status) and np.array_equal(dev.branch[ok], host.branch[ok]) and ok.sum() >= 300
    if what == "ON_EEQOS":
        assert 0 < ((host.branch[ok] & capi.SFR_B_ON_EEQOS) != 0).sum() < ok.sum()
        return
    # get_egyeff: egyhot (1 - x) + cold x with (1 - x) rel T / 2 and x rel T: rel T.  A fraction: cold x + (1 - x) hot with each fraction query
    # rel T (test_gpu_cooling.py's figure for them), x rel T, (1 - x) rel T / 2: at most 2 T cold x + 1.5 T (1 - x) hot <= 2 T of the value.
    assert np.all(np.abs(dev.query[ok] - host.query[ok]) <= (2 * T + R) * np.abs(host.query[ok]))


# ---- (3) shq_sfr_on_eeqos, shq_cooling, shq_starformation end to end -----------------------------------------------------------------------

NGRID = 12
BOXSIZE = 20000.0
ERR_NOMEM = 3


@functools.lru_cache(maxsize=None)
def _zreion_table():
    """5^3, smooth, around the step's redshift: some cells reionise later than it (their rates are zero), some before"""
    i = np.arange(5)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    t = 3.0 + 0.1 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y) + 0.03 * z
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _particles():
    """the layout of test_gpu_cooling.py's end-to-end set: 2 x 12^3 particles, gas and dark matter interleaved at random, a garbage row, a
    zero-mass row, wind particles; about a fifth of the gas is dense (threshold .. 1e3 x threshold) with energies EgySpecCold .. 1e7,
    mixed BHHeated and Generation, masses 0.4 .. 2.5 avg_baryon_mass; one dense particle is BH-heated above the rate table"""
    par = sc.params(avg_baryon_mass=1.0)
    un = sc.case().units
    rng = np.random.default_rng(413)
    ngas = NGRID ** 3
    n = 2 * ngas
    types = rng.permutation(np.concatenate([np.zeros(ngas, np.uint8), np.ones(ngas, np.uint8)]))
    P = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    P["Type"] = types
    P["Pos"] = rng.random((n, 3)) * BOXSIZE
    gi = np.flatnonzero(types == 0)
    P["Mass"] = rng.uniform(0.4, 2.5, n).astype(P["Mass"].dtype)
    P["Hsml"] = rng.uniform(0.5, 5.0, n)
    P["Vel"] = rng.normal(size=(n, 3))
    P["TimeBinHydro"] = rng.integers(15, 20, n)           # bin 15 carries dloga = 0 below
    P["TimeBinHydro"][gi[rng.random(ngas) < 0.1]] = 0
    P["PI"][gi] = rng.permutation(ngas)
    P["Flags"][gi] = ((rng.integers(0, 4, ngas) << 4) | (8 * (rng.random(ngas) < 0.3)) | (4 * (rng.random(ngas) < 0.5))).astype(np.uint8)
    S = np.zeros(ngas, dtype=capi.SPH_DTYPE)
    nphys = 10.0 ** rng.uniform(-7, -2.5, ngas)
    S["Density"] = nphys * cr.PROTONMASS / un.density_in_phys_cgs / sc.A3INV
    temp = 10.0 ** rng.uniform(2.5, 7.5, ngas)
    mu = 4.0 / (1 + 3 * cr.HYDROGEN_MASSFRAC)
    u = temp * cr.BOLTZMANN / (cr.GAMMA_MINUS1 * cr.PROTONMASS * mu) / un.uu_in_cgs
    dense = rng.random(ngas) < 0.2
    S["Density"][dense] = par["PhysDensThresh"] / sc.A3INV * 10.0 ** rng.uniform(0, 3, dense.sum())
    u[dense] = 10.0 ** rng.uniform(np.log10(par["EgySpecCold"]), 7, dense.sum())
    hot = np.flatnonzero(dense)[0]
    u[hot] = 5e7
    S["Entropy"] = u / np.array([cr.entropy_to_u(float(d), sc.A3INV) for d in S["Density"]])
    S["Ne"] = rng.uniform(0, 1.2, ngas)
    S["Metallicity"] = rng.uniform(0, 0.05, ngas)
    S["Sfr"] = rng.uniform(0.1, 1.0, ngas)
    S["DivVel"], S["CurlVel"] = rng.normal(0, 300, ngas), np.abs(rng.normal(0, 300, ngas))
    S["DelayTime"] = np.where(rng.random(ngas) < 0.1, 0.3, 0.0)
    S["DelayTime"][hot] = 0.0
    slot_owner = np.zeros(ngas, dtype=np.int64)
    slot_owner[P["PI"][gi]] = gi
    P["Flags"][slot_owner[hot]] = 8
    P["TimeBinHydro"][slot_owner[hot]] = 18
    P["Flags"][gi[3]] |= 1                                 # garbage
    P["Mass"][gi[4]] = 0                                   # Mass <= 0
    ids = rng.integers(1, 2 ** 56, n, dtype=np.uint64)
    grad = S["Density"] * 10.0 ** rng.uniform(-2, 1, ngas)
    for a in (P, S, ids, grad):
        a.setflags(write=False)
    return P, S, ids, grad, int(slot_owner[hot])


def _step(mode=capi.COOL_UVBG_ZREION):
    case, par = sc.case(), sc.params(avg_baryon_mass=1.0)
    st = capi.CoolingStep()
    st.redshift, st.a3inv, st.hubble = sc.REDSHIFT, sc.A3INV, sc.HUBBLE
    for b in range(capi.TIMEBINS + 1):
        st.kf.dloga_for_bin[b] = 1e-3 if b == 0 else (0.0 if b <= 15 else 4e-3 * 2.0 ** (b - 16))
        st.lastred_for_bin[b] = sc.REDSHIFT
    for k, v in case.uv.items():
        setattr(st.GlobalUVBG, k, v)
    st.uvbg_mode, st.StarformationOn = mode, 1
    st.temp_to_u, st.HIReionTemp, st.MinGasTemp, st.lmfp_heat = par["temp_to_u"], 0.0, 100.0, case.lmfp_heat
    st.CurrentParticleOffset[:] = [0.25 * BOXSIZE, -0.125 * BOXSIZE, 0.0]
    st.PhysDensThresh, st.OverDensThresh = par["PhysDensThresh"], par["OverDensThresh"]
    return st


def _same_records(a, b):
    return all(np.array_equal(a[name], b[name]) for name in a.dtype.names)


def _fresh(ctx):
    P0, S0, ids, grad, _ = _particles()
    pman = sq.PartManager(len(P0), BOXSIZE)
    pman.Base[:] = P0
    sq.cooling_set_tables(ctx, sc.case().tables(zreion=_zreion_table(), zreion_boxsize=BOXSIZE))
    return pman, S0.copy()


def _arrays(P, S, grad, ids, lst, st):
    """the array-level inputs of shq_sfr_eval for the particles of a list"""
    pi = P["PI"][lst]
    dloga = np.array([st.kf.dloga_for_bin[int(b)] for b in P["TimeBinHydro"][lst]])
    return dict(Density=S["Density"][pi], Entropy=S["Entropy"][pi], Ne=S["Ne"][pi], Metallicity=S["Metallicity"][pi], Mass=P["Mass"][lst].astype(np.float64),
                Hsml=P["Hsml"][lst].astype(np.float64), DivVel=S["DivVel"][pi], CurlVel=S["CurlVel"][pi], GradRho=grad[pi], dloga=dloga, DelayTime=S["DelayTime"][pi],
                timebin=P["TimeBinHydro"][lst].astype(np.uint8), flags=P["Flags"][lst].astype(np.uint8), ID=ids[lst])


def _predict(evaluate, what, par, P, S, grad, ids, lst, st):
    """evaluate(what, par, arrays, local_uv) per group of the Zreion mode's local UVBG (get_local_UVBG_from_global: the global one, or
    zero rates where the particle's zreion is below the step's redshift), merged in list order"""
    case = sc.case()
    tab = [float(v) for v in _zreion_table().ravel()]
    off = list(st.CurrentParticleOffset)
    late = np.array([cr.eval_periodic([float(P["Pos"][i][d]) - off[d] for d in range(3)], tab, 5, BOXSIZE) < st.redshift for i in lst])
    assert late.any() and (~late).any()
    a = _arrays(P, S, grad, ids, lst, st)
    dark = cr.make_uvbg(self_shield_dens=case.uv["self_shield_dens"])
    r0, r1 = evaluate(what, par, a, None), evaluate(what, par, a, dark)
    for x, y in zip(r0.arrays(), r1.arrays()):
        x[..., late] = y[..., late]
    return sq.SfrResult(*r0.arrays())


def _restated_eval(what, par, a, uv=None):
    """the Python restatement of sfr_eff.cpp over the arrays, in the shape of a library result"""
    out, flags, decision, branch, ev, left = sc.restated(what, par, a, local_uv=uv)
    return sq.SfrResult(out, flags, decision, branch, np.where(left, capi.COOL_DEFERRED, capi.COOL_OK).astype(np.int32), ev)


def test_on_eeqos_mask_feeds_cooling(sctx):
    """BHFeedbackUseTcool == 2: the device's mask equals the restatement's, and shq_cooling returns the same eeqos list with either"""
    P, S0, ids, grad, _ = _particles()
    par, st = sc.params(avg_baryon_mass=1.0, BHFeedbackUseTcool=2), _step()
    pman, S = _fresh(sctx)
    active = np.ascontiguousarray(np.random.default_rng(6).permutation(len(P))[:3 * len(P) // 4].astype(np.int32))
    mask = sq.sfr_on_eeqos(sctx, pman, S, sc.lib_params(par), st, active=active)
    assert _same_records(pman.Base, P) and _same_records(S, S0)
    gas = active[(P["Type"][active] == 0) & ((P["Flags"][active] & 1) == 0) & (P["Mass"][active] > 0)]
    h = _restated_eval("ON_EEQOS", par, _arrays(P, S0, grad, ids, gas, st))
    want = np.zeros(len(P), dtype=np.uint8)
    want[gas] = (h.branch & capi.SFR_B_ON_EEQOS) != 0
    assert np.all(h.status == capi.COOL_OK) and np.array_equal(mask, want)
    three = np.array([cr.on_eeqos(dict(StarformationOn=1, PhysDensThresh=st.PhysDensThresh, OverDensThresh=st.OverDensThresh), float(S0["Density"][P["PI"][i]]),
                                  float(S0["DelayTime"][P["PI"][i]]), st.a3inv) for i in gas])
    assert 0 < want[gas].sum() < three.sum()        # the fourth clause took some away
    off = _step()
    off.StarformationOn = 0         # "no sfr: normal cooling" (:506)
    assert not sq.sfr_on_eeqos(sctx, pman, S, sc.lib_params(par), off, active=active).any()
    _, e1, _ = sq.cooling(sctx, pman, S, st, active=active, on_eeqos=mask)
    pman2, S2 = _fresh(sctx)
    _, e2, _ = sq.cooling(sctx, pman2, S2, st, active=active, on_eeqos=want)
    assert np.array_equal(e1, e2) and np.array_equal(e1, active[want[active] != 0]) and _same_records(S, S2)


@pytest.mark.parametrize("criterion", [1, 3 | 21])
def test_starformation_end_to_end(sctx, criterion):
    P, S0, ids, grad, i_hot = _particles()
    par, st = sc.params(avg_baryon_mass=1.0, winds_subgrid=1, StarformationCriterion=criterion), _step()
    lp = sc.lib_params(par)
    pman, S = _fresh(sctx)
    active = np.ascontiguousarray(np.random.default_rng(5).permutation(len(P))[:3 * len(P) // 4].astype(np.int32))
    if i_hot not in active:
        active[0] = i_hot
    _, eeqos, _ = sq.cooling(sctx, pman, S, st, active=active)
    assert len(eeqos) > 150 and i_hot in eeqos
    Pc, Sc = pman.Base.copy(), S.copy()
    # what the array-level entry computes for these particles on the device, and the restatement
    dev = _predict(lambda *a: _eval(sctx, *a), "STARFORM", par, Pc, Sc, grad, ids, eeqos, st)
    host = _predict(_restated_eval, "STARFORM", par, Pc, Sc, grad, ids, eeqos, st)     # the restatement's membership of the three lists
    ok = dev.status == capi.COOL_OK
    assert np.array_equal(dev.status, host.status) and list(eeqos[dev.status == capi.COOL_DEFERRED]) == [i_hot] and ok.sum() == len(eeqos) - 1
    assert np.array_equal(dev.decision[ok], host.decision[ok]) and np.array_equal(dev.branch[ok], host.branch[ok])
    assert criterion != 1 or min((dev.decision[ok] == d).sum() for d in (0, 1, 2)) >= 3
    sq.cooling_set_tables(sctx, sc.case().tables(zreion=_zreion_table(), zreion_boxsize=BOXSIZE))
    res, (parents, mos, split), (wind, sm), deferred = sq.starformation(sctx, pman, S, lp, st, eeqos, ids, sc.rnd_table(), GradRho=grad)
    # the records: OK particles as shq_sfr_eval predicts, everything else bit-unchanged
    pi = Pc["PI"][eeqos[ok]]
    for name, row in (("Sfr", dev.Sfr), ("Ne", dev.Ne), ("Metallicity", dev.Metallicity), ("Entropy", dev.Entropy)):
        assert np.array_equal(S[name][pi], row[ok]), name
    assert np.array_equal(pman.Base["Flags"][eeqos[ok]], dev.flags[ok]) and (pman.Base["Flags"][eeqos[ok]] != Pc["Flags"][eeqos[ok]]).any()
    rest = np.ones(len(S), dtype=bool)
    rest[pi] = False
    assert _same_records(S[rest], Sc[rest])
    for name in S.dtype.names:
        if name not in ("Sfr", "Ne", "Metallicity", "Entropy"):
            assert np.array_equal(S[name], Sc[name]), name
    for name in Pc.dtype.names:
        if name != "Flags":
            assert np.array_equal(pman.Base[name], Pc[name]), name
    restp = np.ones(len(Pc), dtype=bool)
    restp[eeqos[ok]] = False
    assert np.array_equal(pman.Base["Flags"][restp], Pc["Flags"][restp])
    # the lists, in list order
    star = ok & (dev.decision != capi.SFR_NONE)
    assert np.array_equal(parents, eeqos[star]) and np.array_equal(mos, dev.mass_of_star[star]) and np.array_equal(split, dev.decision[star] == capi.SFR_SPLIT)
    nostar = ok & (dev.decision == capi.SFR_NONE)
    assert np.array_equal(wind, eeqos[nostar]) and np.array_equal(sm, dev.sm[nostar]) and list(deferred) == [i_hot]
    assert (res.n_newstars, res.n_split, res.n_maybewind, res.n_deferred, res.sum_sf_part) == (star.sum(), (dev.decision[ok] == capi.SFR_SPLIT).sum(), nostar.sum(), 1, ok.sum())
    assert list(res.n_status) == [ok.sum(), 1, 0, 0] and res.n_skipped == 0 and res.kernel_ms > 0 and res.steps == int(dev.steps.sum())
    # the sums: left to right in list order over the device's addends, bit for bit
    for got, row in ((res.localsfr, dev.Sfr), (res.sum_sm, dev.dM), (res.sum_dtime, dev.dtime)):
        acc = 0.0
        for v in row[ok]:
            acc += float(v)
        assert got == acc
    # the context's copy of the entropies equals the caller's records
    gas = np.flatnonzero(Pc["Type"] == 0)
    assert np.array_equal(sq.entropy_download(sctx, len(Pc))[gas], S["Entropy"][Pc["PI"][gas]])
    # a short capacity: SHQ_ERR_NOMEM after everything else has been written, the counts are right
    pman2, S2 = _fresh(sctx)
    sq.cooling(sctx, pman2, S2, st, active=active)
    with pytest.raises(sq.ShqError) as e:
        sq.starformation(sctx, pman2, S2, lp, st, eeqos, ids, sc.rnd_table(), GradRho=grad, capacity=3)
    assert f"status {ERR_NOMEM}" in str(e.value)
    r2 = e.value.result
    assert (r2.n_newstars, r2.n_maybewind, r2.n_deferred) == (res.n_newstars, res.n_maybewind, 1) and _same_records(S2, S) and _same_records(pman2.Base, pman.Base)
    # under shq_set_inputs_current the call reads the context's copies, which shq_cooling left current
    pman3, S3 = _fresh(sctx)
    sq.cooling(sctx, pman3, S3, st, active=active)
    capi.check(capi.hip.shq_set_inputs_current(sctx.h, capi.CURRENT_PARTICLES | capi.CURRENT_SPH))
    res3, l3, w3, d3 = sq.starformation(sctx, pman3, S3, lp, st, eeqos, ids, sc.rnd_table(), GradRho=grad)
    capi.check(capi.hip.shq_set_inputs_current(sctx.h, 0))
    assert _same_records(S3, S) and _same_records(pman3.Base, pman.Base) and np.array_equal(l3[0], parents) and np.array_equal(w3[1], sm)
    assert (res3.localsfr, res3.sum_sm, res3.sum_dtime) == (res.localsfr, res.sum_sm, res.sum_dtime)


def test_starformation_quick_lyman_alpha(sctx):
    """the call classifies the active list itself; every hit converts the parent with sm = Mass and nothing is written"""
    P, S0, ids, grad, _ = _particles()
    par, st = sc.params(avg_baryon_mass=1.0, QuickLymanAlphaProbability=0.5, QuickLymanAlphaTempThresh=1e5, OverDensThresh=float(np.quantile(S0["Density"], 0.5))), _step()
    pman, S = _fresh(sctx)
    active = np.ascontiguousarray(np.random.default_rng(7).permutation(len(P))[:3 * len(P) // 4].astype(np.int32))
    res, (parents, mos, split), (wind, sm), deferred = sq.starformation(sctx, pman, S, sc.lib_params(par), st, active, ids, sc.rnd_table())
    assert _same_records(S, S0) and _same_records(pman.Base, P)
    gas = active[(P["Type"][active] == 0) & ((P["Flags"][active] & 1) == 0) & (P["Mass"][active] > 0)]
    h = _restated_eval("STARFORM", par, _arrays(P, S0, grad, ids, gas, st))
    hit = h.decision == 1
    assert np.all(h.status == capi.COOL_OK) and 20 < hit.sum() < len(gas) - 20
    assert np.array_equal(parents, gas[hit]) and np.array_equal(mos, P["Mass"][gas[hit]].astype(np.float64)) and not split.any() and len(wind) == 0 and len(deferred) == 0
    acc = 0.0
    for v in P["Mass"][gas[hit]]:
        acc += float(v)
    assert res.sum_sm == acc and res.sum_sf_part == hit.sum() and res.localsfr == 0 and res.sum_dtime == 0 and res.n_skipped == len(active) - len(gas)


def test_eval_leaves_the_cached_ids_alone(sctx):
    """under SHQ_CURRENT_IDS the context keeps its copy of the caller's IDs by particle index; shq_sfr_eval, which takes IDs in list order
    for another number of particles, must not disturb it: shq_starformation before and after gives the same draws"""
    P, S0, ids, grad, _ = _particles()
    par, st = sc.params(avg_baryon_mass=1.0, winds_subgrid=1), _step()
    lp = sc.lib_params(par)
    active = np.ascontiguousarray(np.random.default_rng(5).permutation(len(P))[:3 * len(P) // 4].astype(np.int32))

    def run():
        pman, S = _fresh(sctx)
        _, eeqos, _ = sq.cooling(sctx, pman, S, st, active=active)
        res, new, wind, deferred = sq.starformation(sctx, pman, S, lp, st, eeqos, ids, sc.rnd_table(), GradRho=grad)
        return pman, S, eeqos, res, new, wind, deferred

    try:
        capi.check(capi.hip.shq_set_inputs_current(sctx.h, capi.CURRENT_IDS))
        a = run()
        eeqos = a[2]
        pred = _eval(sctx, "STARFORM", par, _arrays(P, S0, grad, ids, eeqos[:97], st))       # 97 IDs in list order
        assert np.all(pred.status[pred.status != capi.COOL_DEFERRED] == capi.COOL_OK)
        b = run()
    finally:
        capi.check(capi.hip.shq_set_inputs_current(sctx.h, 0))
    c = run()           # and with the IDs uploaded afresh
    for x in (b, c):
        assert _same_records(x[1], a[1]) and _same_records(x[0].Base, a[0].Base)
        assert all(np.array_equal(u, v) for u, v in zip(x[4] + x[5] + (x[6],), a[4] + a[5] + (a[6],)))
        assert (x[3].localsfr, x[3].sum_sm, x[3].n_newstars) == (a[3].localsfr, a[3].sum_sm, a[3].n_newstars)
    assert a[3].n_newstars >= 3
