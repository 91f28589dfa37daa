"""Linear-response neutrinos without a GPU: the restatement (tests/nulra_restated.py) against the reference's own unit-test gates, the
host engine (shq_nulra_host_*, the code the device runs, driven in plain loops) against the restatement, the state machine of
delta_nu_from_power, and the host engine as a stand-alone program (the one the host sanitizers are run on)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import shenqi_amd as sq
import nulra_restated as nr
import nulra_cases as nc

ERR_INVALID, ERR_DEVICE, ERR_STATE = 1, 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement passes the reference's gates (libgadget/tests/test_neutrinos_lra.cpp) ----

def test_restated_specialJ_gates():
    """:102-112, value and relative tolerance"""
    cases = [((0, -1, 0), 1.0, 0.0), ((1, -1, 0), 0.2117, 1e-3), ((2, -1, 0), 0.0223807, 1.2e-2), ((0.5, -1, 0), 0.614729, 1e-3), ((0.3, -1, 0), 0.829763, 1e-3),
             ((0, 1, 0), 0.940437, 1e-4), ((0.5, 1e-2, 0.5), 0.614729 / 0.5, 1.3e-4), ((0.5, 1, 0.5), 0.556557 / 0.5, 1e-2), ((1, 0.1, 0.5), 0.211662 / 0.5, 1e-4)]
    for (x, qc, nf), want, tol in cases:
        got = float(nr.specialJ(np.array([float(x)]), qc, nf)[0])
        assert abs(got - want) <= tol * abs(want), (x, qc, nf, got, want)


def test_restated_fslength_gates():
    """:135-138 with the Mathematica snippet's H(a) (:118-124); the deviations are -2.9e-6 and -5.9e-7"""
    c = nc.cosmo("equal")
    for (ai, af), want in (((0.5, 1.0), 1272.92 * (0.45 / nr.KBTNU)), ((0.1, 0.5), 5427.8 * (0.6 / nr.KBTNU))):
        got = nr.fslength(c.hubble, np.log(ai), np.log(af), 299792.0)
        print("fslength", ai, af, got / want - 1)
        assert abs(got / want - 1) < 1e-5


def _few_timesteps(ia):
    k = 0.01 * 10.0 ** (3.0 * np.arange(10) / 9)
    a = 0.01 * (1 + 0.5 * np.arange(ia + 1))
    return dict(ia=ia + 1, nk=10, scalefact=np.log(a), delta_tot=np.ascontiguousarray(np.tile(1e-3 * (a / 0.01), (10, 1))), delta_nu_init=np.full(10, 1e-3),
                kvalue=k), float(a[-1])


@pytest.mark.parametrize("ia", [1, 2, 3, 4])
def test_few_timesteps(ia):
    """test_get_delta_nu_few_timesteps (:64-95): finite and below 1 at table sizes 2 .. 5, for the restatement and for the host engine"""
    st, a = _few_timesteps(ia)
    c = nc.cosmo("equal")
    r = nr.get_delta_nu(c, 0.01, st["scalefact"], st["delta_tot"], st["kvalue"], st["delta_nu_init"], a, 0.15)
    assert np.isfinite(r).all() and (np.abs(r) < 1).all()
    with nc.make(None, c) as nu:
        nu.set_state(st)
        d = nu.delta_nu(a)
    assert np.isfinite(d).all() and (np.abs(d) < 1).all()
    assert nc.rel(d, nr.get_delta_nu_combined(c, 0.01, st["scalefact"], st["delta_tot"], st["kvalue"], st["delta_nu_init"], a)) < nc.GATE


# ---- 2. the host engine against the restatement ----

@pytest.mark.parametrize("Na", nc.NAS)
@pytest.mark.parametrize("name", nc.COSMOS)
def test_host_engine_against_restatement(name, Na):
    """Every delta_nu entry within sqrt(epsilon) relative.  Measured worst deviations: 4.5e-11 (equal and mixed masses, every Na),
    3.6e-13 (hybrid), 2.2e-16 at Na = 1 (the initial-condition piece alone)."""
    c = nc.cosmo(name)
    st = nc.history(Na)
    with nc.make(None, c) as nu:
        nu.set_state(st)
        d = nu.delta_nu(float(np.exp(st["scalefact"][-1])))
        nodes = nu.info().nnodes
    ref = nc.restated_delta_nu(c, st)
    worst = nc.rel(d, ref)
    print(f"nulra host vs restatement: {name} Na {Na}: worst {worst:.3e}, {nodes} nodes")
    assert d.shape == (10,) and worst < nc.GATE
    if name == "hybrid" and Na > 1:
        assert nodes > 50000   # the truncated J's phase is resolved
    if name == "mixed" and Na > 1:
        # the massless species contributes its initial-condition piece alone: dropping it changes the answer
        c2 = nr.Cosmo([0.2, 0.05, 0.0], [1, 1, 0])
        assert nc.rel(nc.restated_delta_nu(c2, st), ref) > 1e-6


# ---- 3. the state machine ----

KEPT = [-1, 0, 0, 1, -1, 1, 1, 0, 1, 1, 1, 1]   # nc.TIMES under the 0.009 rule, -1: no update (first call at TimeIC, repeated Time)


def _check_against(nu_steps, ref_steps):
    for (info, d, st), (ria, rkept, rd, rdt, rsf) in zip(nu_steps, ref_steps):
        assert info.ia == ria == st["ia"] and info.kept == rkept
        assert nc.rel(st["scalefact"], rsf) < 1e-15
        assert nc.rel(d, rd) < nc.GATE
        assert nc.rel(st["delta_tot"], rdt) < nc.GATE


def _sequence(nu, ref, times=nc.TIMES):
    k, nm = nc.bins()
    a_steps, r_steps = [], []
    for t in times:
        s = nc.sums(k, nm, t)
        nu.step(t, nc.TIME_TRANSFER, sq.pack_sums(*s))
        ref.step(t, nc.TIME_TRANSFER, *s)
        d, kk, info = nu.download()
        assert nc.rel(kk, k) < 1e-14 and info.nonzero == len(k)
        a_steps.append((info, d, nu.get_state()))
        r_steps.append((ref.ia, ref.kept, ref.delta_nu_last[:ref.nk].copy(), ref.delta_tot[:ref.nk, :ref.ia].copy(), ref.scalefact[:ref.ia].copy()))
    return a_steps, r_steps


@pytest.fixture(scope="module")
def host_run():
    """the twelve steps on the host engine and on the restatement, and both mode tables at Nmesh 16"""
    c = nc.cosmo("equal_mpc")
    ref = nc.restated(c)
    with nc.make(None, c) as nu:
        a, r = _sequence(nu, ref)
        T, T0 = nu.mode_table(16), nu.mode_table(16, add_one=False)
        prefac = nu.info().nu_prefac
    return a, r, T, T0, ref.mode_table(16), prefac, ref


def test_keep_or_discard_sequence(host_run):
    a, r, *_ = host_run
    assert [s[0].kept for s in a] == KEPT
    assert a[-1][0].ia == 8 and a[0][0].ia == 1
    _check_against(a, r)


def test_mode_table_nmesh16(host_run):
    """193 entries; k(k2 = 1) = 1 lies below the first knot (k = 2) and k(k2 = 192) = 13.9 beyond the last (10): the end knots' values"""
    a, r, T, T0, Tref, prefac, ref = host_run
    assert T.shape == (193,) and T[0] == 1.0 and T0[0] == 0.0
    assert nc.rel(T, Tref) < nc.GATE
    assert nc.rel(T0[1:], Tref[1:] - 1) < 1e-6 and np.array_equal(T0[1:] + 1.0, T[1:])
    assert nc.rel(prefac, ref.nu_prefac) < 1e-14
    assert T[1] == T[2] == T[3] and nc.rel(T0[1], prefac * ref.ratio[0]) < nc.GATE            # k2 = 1, 2, 3: k < 2
    assert T[101] == T[150] == T[192] and nc.rel(T0[192], prefac * ref.ratio[-1]) < nc.GATE   # k2 > 100: k > 10
    assert (T[5:100] != T[1]).all()


def test_repeated_time_refreshes_the_table_only():
    c = nc.cosmo("equal_mpc")
    k, nm = nc.bins()
    with nc.make(None, c) as nu:
        for t in (0.01, 0.022, 0.035):
            nu.step(t, 0.01, sq.pack_sums(*nc.sums(k, nm, t)))
        st0, (d0, _, i0), T0 = nu.get_state(), nu.download(), nu.mode_table(16, add_one=False)
        kk, power, nmodes, norm = nc.sums(k, nm, 0.035)
        nu.step(0.035, 0.01, sq.pack_sums(kk, 4 * power, nmodes, norm))   # the same Time, twice the delta_cdm
        st1, (d1, _, i1), T1 = nu.get_state(), nu.download(), nu.mode_table(16, add_one=False)
    assert i1.kept == -1 and i1.ia == i0.ia == 3
    for key in ("scalefact", "delta_tot", "delta_nu_init", "kvalue"):
        assert np.array_equal(st0[key], st1[key])
    assert np.array_equal(d0, d1)
    assert (T0[1:] > 0).all() and nc.rel(T1[1:], T0[1:] / 2) < 1e-12    # delta_nu / Power_in halves


def test_all_particles_skips_the_update():
    """1 - partnu < 1e-3 past nu_crit_time: no history update, and get_delta_nu is the initial-condition piece alone"""
    c = nc.cosmo("allparticles")
    ref = nc.restated(c)
    with nc.make(None, c) as nu:
        a, r = _sequence(nu, ref, times=(0.01, 0.022, 0.035, 0.05))
    assert [s[0].kept for s in a] == [-1, 1, -1, -1] and a[-1][0].ia == 2
    _check_against(a, r)


def _rebin_state():
    st = nc.history(6, nk=7)
    st["kvalue"] = np.array([1.0, 2.0, 2.9, 4.4, 6.1, 10.0, 14.0])   # below, on, inside, on and beyond the sums' bins k = 2 .. 10
    st["scalefact"] = np.log(0.01 * 5 ** (np.arange(6) / 5.0))        # a = 0.01 .. 0.05
    return st


def test_rebin_branch():
    """nk = 7 differs from the 10 non-empty bins: Power_in rebinned in log space (a k outside the bins takes the last delta_tot), the
    ratio rebinned back; two of twelve bins are empty"""
    c = nc.cosmo("equal_mpc")
    st = _rebin_state()
    k, nm = nc.bins(12, empty=(3, 7))
    ref = nc.restated(c)
    ref.ia, ref.nk = 6, 7
    ref.scalefact[:6], ref.delta_tot[:7, :6], ref.delta_nu_init[:7], ref.wavenum[:7] = st["scalefact"], st["delta_tot"], st["delta_nu_init"], st["kvalue"]
    with nc.make(None, c) as nu:
        nu.set_state(st)
        for t in (0.07, 0.1):
            s = nc.sums(k, nm, t)
            nu.step(t, 0.01, sq.pack_sums(*s))
            ref.step(t, 0.01, *s)
        d, kk, info = nu.download()
        T = nu.mode_table(16)
        st1 = nu.get_state()
    assert info.nk == 7 and info.nonzero == 10 and info.ia == 8 == ref.ia
    assert nc.rel(kk, k[nm != 0]) < 1e-14
    assert nc.rel(d, ref.delta_nu_last[:7]) < nc.GATE
    assert nc.rel(st1["delta_tot"], ref.delta_tot[:7, :8]) < nc.GATE
    assert nc.rel(T, ref.mode_table(16)) < nc.GATE


def test_negative_clamp():
    c = nc.cosmo("equal_mpc")
    st = nc.history(4)
    st["delta_nu_init"][:2] = -10.0   # a huge negative initial-condition piece in the two bins of the smallest k
    k, nm = nc.bins()
    with nc.make(None, c) as nu:
        nu.set_state(st)
        raw = nu.delta_nu(float(np.exp(st["scalefact"][-1])))
        nu.step(0.5, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.5)))   # the same Time as the last stored spectrum: no update, the clamp alone
        d, _, info = nu.download()
    assert (raw[:2] < 0).all() and (raw[2:] > 0).all()
    assert info.kept == -1 and (d[:2] == 0).all() and np.array_equal(d[2:], raw[2:])


def test_nan_gives_the_error_code():
    c = nc.cosmo("equal_mpc")
    st = nc.history(5)
    st["delta_tot"][3, 2] = np.nan
    k, nm = nc.bins()
    with nc.make(None, c) as nu:
        nu.set_state(st)
        assert nu.try_step(0.6, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.6))) == ERR_DEVICE
        assert nu.try_step(0.7, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.7))) == ERR_DEVICE   # sticky
        with pytest.raises(sq.capi.ShqError):
            nu.mode_table(16)


def test_state_round_trip_is_bit_exact():
    """get_state -> set_state into a fresh engine: the next step is the same to the bit; without delta_nu_last (the reference's snapshot
    block) the restored engine recomputes it from the final history, so the next step agrees to the quadrature's accuracy only"""
    c = nc.cosmo("mixed_mpc")
    k, nm = nc.bins()
    nxt = sq.pack_sums(*nc.sums(k, nm, 0.07))
    with nc.make(None, c) as nu:
        for t in (0.01, 0.022, 0.035, 0.05):
            nu.step(t, 0.01, sq.pack_sums(*nc.sums(k, nm, t)))
        st = nu.get_state()
        nu.step(0.07, 0.01, nxt)
        want, (dwant, _, iwant), Twant = nu.get_state(), nu.download(), nu.mode_table(16)
    assert st["ia"] == 4 and st["delta_tot"].shape == (10, 4)
    with nc.make(None, c) as fresh:
        fresh.set_state(st)
        fresh.step(0.07, 0.01, nxt)
        got, (dgot, _, igot), Tgot = fresh.get_state(), fresh.download(), fresh.mode_table(16)
    assert igot.ia == iwant.ia == 5 and igot.kept == iwant.kept == 1
    for key in ("scalefact", "delta_tot", "delta_nu_init", "kvalue", "delta_nu_last"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(dgot, dwant) and np.array_equal(Tgot, Twant)
    with nc.make(None, c) as snap:
        snap.set_state({key: v for key, v in st.items() if key != "delta_nu_last"})
        snap.step(0.07, 0.01, nxt)
        d3 = snap.download()[0]
    assert nc.rel(d3, dwant) < 1e-3 and not np.array_equal(d3, dwant)


def test_set_state_limits_and_errors():
    """petaio_read_neutrinos' endrun(5): nk > nk_allocated or ia > namax; too few bins; a k beyond the transfer table"""
    c = nc.cosmo("equal_mpc")
    with nc.make(None, c, nk_allocated=12, TimeMax=0.05) as nu:   # namax = ceil(0.04 / 0.008) + 4 = 9
        assert nu.info().namax == 9
        assert nu.try_set_state(nc.history(9)) == 0
        assert nu.try_set_state(nc.history(10)) == ERR_INVALID
        assert nu.try_set_state(nc.history(4, nk=13)) == ERR_INVALID
        k, nm = nc.bins(3)
        assert nu.try_step(0.02, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.02))) == ERR_INVALID
    with nc.make(None, c) as nu:
        k, nm = nc.bins(10, kmax=2000.0)
        assert nu.try_step(0.01, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.01))) == ERR_INVALID
    with nc.make(None, c, nk_allocated=8) as nu:
        k, nm = nc.bins(10)
        assert nu.try_step(0.01, 0.01, sq.pack_sums(*nc.sums(k, nm, 0.01))) == ERR_INVALID   # 10 non-empty bins, 8 allocated


def test_first_init_from_the_transfer_table():
    """delta_tot_first_init (:99-134): delta_nu_init = delta_cdm T_nu(log10 k) with the table's makima, the first delta_tot, scalefact[0]"""
    c = nc.cosmo("mixed_mpc")
    ref = nc.restated(c)
    k, nm = nc.bins(12, empty=(0, 5))
    s = nc.sums(k, nm, 0.012)
    with nc.make(None, c) as nu:
        nu.step(0.012, 0.012, sq.pack_sums(*s))
        st = nu.get_state()
    ref.step(0.012, 0.012, *s)
    assert st["ia"] == 1 and st["nk"] == 10 and st["scalefact"][0] == np.log(0.012)
    assert nc.rel(st["kvalue"], k[nm != 0]) < 1e-14
    assert nc.rel(st["delta_nu_init"], ref.delta_nu_init[:10]) < 1e-13
    assert nc.rel(st["delta_tot"][:, 0], ref.delta_tot[:10, 0]) < 1e-13


# ---- 4. the host side stand-alone ----

def test_standalone_host_program(tmp_path):
    """csrc/nulra_host.hip builds with the plain host compiler beside a main of its own (tools/nulra_host_main.cpp, the program the
    sanitizers are run on: its header has the command) and that program passes: first init, twelve steps, the rebin branch, hybrid steps,
    a bit-equal state round trip, the mode table"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "nulra_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "shenqi_amd", "csrc"),
           os.path.join(ROOT, "tools", "nulra_host_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "nulra standalone ok" in out.stdout, out.stdout + out.stderr
