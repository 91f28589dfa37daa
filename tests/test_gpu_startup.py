"""Run start-up on the device (csrc/startup.hip) against the restatements of startup_restated.py on its shared cases.

Records and slots are compared as bytes, the spare bytes behind them included.  The doubles that pass through the device's pow, which may
differ from glibc's by an ulp, have the project's allowance: 4 x 2^-52 relative for len * pow(...) in set_init_hsml (one multiplication
around the pow; the roundings inside its argument move the result by less than an ulp), 5 x 2^-52 for GAMMA_MINUS1 * u / pow(X / a3,
GAMMA_MINUS1) (test_gpu_snapshot.py's 4 x 2^-52 for this expression, and (2/3) 2^-53 for the extra quotient inside the pow)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shenqi_amd as sq
from shenqi_amd import capi
import common as cm
import startup_restated as st

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_INVALID = 1
POW4, POW5 = 4 * 2.0 ** -52, 5 * 2.0 ** -52
WHICH = (st.OMEGA, st.POSITIONS, st.HSML, st.INIT, st.OMEGA | st.POSITIONS | st.HSML | st.INIT)


def dev(a, spare=2):
    """the records as device bytes, with `spare` more records of a pattern behind them"""
    raw = a.view(np.uint8).reshape(-1)
    raw = np.concatenate([raw, np.full(spare * a.dtype.itemsize + 16, 0xA5, dtype=np.uint8)])
    return torch.from_numpy(raw).to(DEV)


def same_bytes(d, want, spare=2):
    got = d.cpu().numpy()
    n = want.nbytes
    return np.array_equal(got[:n], want.view(np.uint8).reshape(-1)) and np.all(got[n:] == 0xA5) and len(got) == n + spare * want.dtype.itemsize + 16


def status_of(call):
    try:
        call()
    except capi.ShqError as e:
        return int(str(e).split("status ")[1].split(":")[0])
    return 0


def c_params(par):
    return sq.startup_params(par.BoxSize, par.MassTable, par.MeanSeparation, par.Ti_Current, par.generations, par.RestartSnapNum, par.init_reion)


def run_particles(ctx, k, par, which):
    L = sq.startup_layout(sph_dtype=k.S.dtype)
    dP, dS, dB = dev(k.P), dev(k.S), dev(k.B)
    rep = sq.startup_particles(ctx, L, dP, k.n, dS, len(k.S), dB, len(k.B), c_params(par), which)
    return dP, dS, dB, rep


# ---- (1) the record loops ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", st.COUNTS)
def test_record_loops_equal_the_restatement(ctx, n):
    for reion in ((True, False) if n == 257 else (True,)):
        k = st.case(n, reion)
        for mode in ("ic", "restart") + (("restart_reion",) if n == 257 else ()):
            par = st.MODES[mode]
            for which in WHICH:
                P, S, B, want = st.particles(k.P, k.S, k.B, par, which)
                dP, dS, dB, rep = run_particles(ctx, k, par, which)
                tag = (n, reion, mode, which)
                assert same_bytes(dP, P), tag
                assert same_bytes(dS, S), tag
                assert same_bytes(dB, B), tag
                for f in ("badmass", "noutside", "first_outside", "numzero", "lastzero", "numprob", "lastprob", "nbad_delaytime", "first_bad_delaytime"):
                    assert getattr(rep, f) == want[f], (tag, f)
                if not which & st.OMEGA:
                    assert rep.mass_total == 0 and not rep.mass_type.any()
                    continue
                # any summation order is within (n - 1) 2^-53 sum |m| of the exact sum (the reference's own order under OpenMP is unspecified)
                for got, m in zip(list(rep.mass_type) + [rep.mass_total], want["mass_type"] + [want["mass_all"]]):
                    bound = max(len(m) - 1, 0) * 2.0 ** -53 * math.fsum(abs(x) for x in m)
                    assert abs(got - math.fsum(m)) <= bound, (tag, got, math.fsum(m), bound)
                again = run_particles(ctx, k, par, which)[3]
                assert again.mass_total.hex() == rep.mass_total.hex() and again.mass_type.tobytes() == rep.mass_type.tobytes(), tag


def test_record_loops_raise_the_reference_messages(ctx):
    k = st.case(65)
    L = sq.startup_layout(sph_dtype=k.S.dtype)
    args = (dev(k.P), k.n, dev(k.S), len(k.S), dev(k.B), len(k.B), c_params(st.MODES["ic"]))
    with pytest.raises(sq.StartupError, match=r"Particle 3 is outside the box \(L=20000\) at \(-1e-300 5 6\)"):
        sq.startup_particles(ctx, L, *args, which=st.POSITIONS, raise_on=True)
    with pytest.raises(sq.StartupError, match=r"Bad DelayTime for part \d+ id \d+"):     # the loop has set DelayTime = 0 by then
        sq.startup_particles(ctx, L, *args, which=st.INIT, raise_on=True)
    restart = (dev(k.P), k.n, dev(k.S), len(k.S), dev(k.B), len(k.B), c_params(st.MODES["restart"]))
    with pytest.raises(sq.StartupError, match=r"Bad DelayTime (nan|-inf) for part \d+ id \d+"):
        sq.startup_particles(ctx, L, *restart, which=st.INIT, raise_on=True)
    P = k.P.copy()
    P["Pos"] = 0.5 * st.BOXSIZE
    P["Pos"][[7, 40]] = 0
    with pytest.raises(sq.StartupError, match="Particle positions contain 2 zeros at particle 40. Pos 0 0 0. Likely write corruption!"):
        sq.startup_particles(ctx, L, dev(P), *args[1:], which=st.POSITIONS, raise_on=True)


@pytest.mark.parametrize("ptype", [0, 5])
def test_a_slot_index_out_of_range_is_refused_before_anything_is_written(ctx, ptype):
    k = st.case(257)
    L = sq.startup_layout(sph_dtype=k.S.dtype)
    for bad in (-1, len(k.slots[ptype])):
        P = k.P.copy()
        P["PI"][np.flatnonzero(P["Type"] == ptype)[-1]] = bad
        dP, dS, dB = dev(P), dev(k.S), dev(k.B)
        call = lambda: sq.startup_particles(ctx, L, dP, k.n, dS, len(k.S), dB, len(k.B), c_params(st.MODES["ic"]), st.OMEGA | st.INIT)  # noqa: E731
        assert status_of(call) == ERR_INVALID
        assert same_bytes(dP, P) and same_bytes(dS, k.S) and same_bytes(dB, k.B)
        # the loops that touch no slot do not look at PI
        sq.startup_particles(ctx, L, dP, k.n, dS, len(k.S), dB, len(k.B), c_params(st.MODES["ic"]), st.OMEGA | st.POSITIONS | st.HSML)


@pytest.mark.parametrize("n", st.COUNTS[1:])
def test_check_density_entropy_equals_the_restatement(ctx, n):
    S = st.entropy_case(n)
    want, bad, raised = st.check_density_entropy(S, st.MEANBAR, st.MINEGYSPEC, st.ATIME)
    dS = dev(S)
    got_bad = sq.check_density_entropy(ctx, sq.startup_layout(), dS, n, st.MEANBAR, st.MINEGYSPEC, st.ATIME)
    assert got_bad == bad
    got = dS.cpu().numpy()[:S.nbytes].view(S.dtype)
    changed = np.flatnonzero(got["Entropy"] != S["Entropy"])
    assert np.array_equal(changed, raised)
    rel = np.abs(got["Entropy"][raised] / want["Entropy"][raised] - 1)
    print("check_density_entropy n=%d: %d raised, max relative difference %.3g" % (n, len(raised), rel.max() if len(raised) else 0))
    assert np.all(rel <= POW5)
    patched = st.bytes_copy(got)
    patched["Entropy"][raised] = want["Entropy"][raised]
    assert np.array_equal(patched.view(np.uint8), want.view(np.uint8)) and np.all(dS.cpu().numpy()[S.nbytes:] == 0xA5)


# ---- (2) shq_set_init_hsml --------------------------------------------------------------------------------------------------------------

def upload(ctx, pman):
    pv = pman.view()
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)), "particles_upload")
    sq.dynamics_upload(ctx, pman)


def device_hsml(ctx, pman, mean, des):
    """shq_set_init_hsml on the resident particles: (Hsml by particle, nodes, status)"""
    status, nodes = 0, None
    try:
        nodes = sq.set_init_hsml_device(ctx, pman.NumPart, mean, des)
    except capi.ShqError as e:
        status, nodes = int(str(e).split("status ")[1].split(":")[0]), e.nodes
    out = sq.PartManager(pman.NumPart, pman.BoxSize)
    out.Base[:] = pman.Base
    sq.dynamics_download(ctx, out)
    return out.Base["Hsml"].copy(), nodes, status


@pytest.mark.parametrize("ngas,mean", [(16 ** 3, 0.5), (12, 0.5), (16 ** 3, 1e-6)])
@pytest.mark.parametrize("built", ["device", "host"])
def test_set_init_hsml_equals_the_restatement(ctx, ngas, mean, built):
    """Particles that end on the root meet the reference's "Bad tree moments" (the root is 1.001 BoxSize long): the call then returns
    SHQ_ERR_INVALID after every Hsml has been written, so both are checked.  In the 16^3 set the sparse octants hold less than
    10 DesNumNgb masses, so some climbs end on the root there too; with 12 particles all do."""
    pman, _, _ = st.hsml_set(ngas)
    n = pman.NumPart
    sq.set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=0.5, DensityKernelType=1, BlackHoleNgbFactor=2.0, MinGasHsml=0.006)
    des = sq.GetNumNgb()
    upload(ctx, pman)
    if built == "device":
        sq.tree_build_device(ctx, pman.BoxSize, sq.GASMASK + sq.BHMASK)
        nodes, father = sq.tree_download(ctx, n, n)
        firstnode = n
    else:
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)
        tv = tree.view()
        capi.check(capi.hip.shq_tree_upload(ctx.h, C.byref(tv)), "tree_upload")
        nodes, father, firstnode = tree.Nodes_base, st.tree_father(tree, n), tree.firstnode
    want, wnodes, badmom, badhsml = st.set_init_hsml(nodes, firstnode, father, pman.Base, mean, des, pman.BoxSize)
    got, gnodes, status = device_hsml(ctx, pman, mean, des)
    assert np.array_equal(gnodes, wnodes)
    assert status == (ERR_INVALID if badmom or badhsml else 0)
    P = pman.Base
    touched = ((P["Type"] == 0) | (P["Type"] == 5)) & ((P["Flags"] & 1) == 0)
    assert touched.sum() == n - 1 and got[~touched].tobytes() == P["Hsml"][~touched].tobytes()
    rel = np.abs(got[touched] / want[touched] - 1)
    print("set_init_hsml %s tree, %d gas: max relative difference %.3g, %d on the root" % (built, ngas, rel.max(), badmom))
    assert np.all(rel <= POW4)
    assert got[n - 1] == mean and gnodes[n - 1] == n - 1      # the swallowed black hole
    if ngas == 12:
        assert badmom == n - 2 and np.all(gnodes[touched][:-1] == firstnode)
    if mean == 1e-6:
        assert np.all(got[touched] == mean)


# ---- (3) shq_init_entropy ---------------------------------------------------------------------------------------------------------------

def gas_only(n, seed):
    rng = np.random.default_rng([st.SEED, n, seed])
    pman, SphP, BhP = cm.make_gas(rng.uniform(0, cm.BOX, (n, 3)), np.full(n, 0.3))
    SphP["Density"] = np.exp(rng.normal(0, 4, n))
    SphP["EgyWtDensity"] = np.exp(rng.normal(0, 4, n))
    return pman, SphP


def upload_sph(ctx, pman, SphP):
    pv, sv = pman.view(), capi.sph_view(SphP)
    capi.check(capi.hip.shq_particles_upload(ctx.h, C.byref(pv)), "particles_upload")
    capi.check(capi.hip.shq_sph_state_upload(ctx.h, C.byref(pv), C.byref(sv)), "sph_state_upload")


@pytest.mark.parametrize("n", [1, 65, 4096])
@pytest.mark.parametrize("from_egywt", [False, True])
def test_init_entropy_equals_numpy(ctx, n, from_egywt):
    pman, SphP = gas_only(n, 3)
    u, a3 = 37.5, 0.25 ** 3
    upload_sph(ctx, pman, SphP)
    sq.init_entropy(ctx, u, a3, from_egywt)
    got = sq.entropy_download(ctx, n)
    X = SphP["EgyWtDensity" if from_egywt else "Density"]
    want = st.GAMMA_MINUS1 * u / np.power(X / a3, st.GAMMA_MINUS1)
    rel = np.abs(got / want - 1)
    print("init_entropy n=%d from_egywt=%d: max relative difference %.3g" % (n, from_egywt, rel.max()))
    assert np.all(rel <= POW5)


# ---- (4) shq_setup_smoothinglengths against the composition of its pieces -------------------------------------------------------------------

U_INIT, ATIME = 37.5, 0.25


def density_call(ctx, pman, SphP, BhP, update_hsml, DoEgy):
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)
    return sq.density(ctx, None, update_hsml, DoEgy, 1, None, tree, pman, SphP, BhP)[1]


def composed(ctx, pman, SphP, BhP, mean, disph):
    """setup_smoothinglengths from pieces tested above: shq_set_init_hsml (downloaded), the one-shot density, shq_init_entropy
    (downloaded) per round and numpy's max"""
    P = pman.Base
    des, a3 = sq.GetNumNgb(), ATIME ** 3
    target = np.flatnonzero(((P["Type"] == 0)) & ((P["Flags"] & 3) == 0))
    upload(ctx, pman)
    sq.tree_build_device(ctx, pman.BoxSize, sq.GASMASK + sq.BHMASK)
    hsml, _, _ = device_hsml(ctx, pman, mean, des)
    P["Hsml"] = hsml
    first = density_call(ctx, pman, SphP, BhP, 1, 0)

    def entropy(from_egywt):
        upload_sph(ctx, pman, SphP)
        sq.init_entropy(ctx, U_INIT, a3, from_egywt)
        SphP["Entropy"][P["PI"][target]] = sq.entropy_download(ctx, pman.NumPart)[target]

    maxdiffs, rounds = [], 0
    if not disph:
        entropy(False)
        return first, rounds, maxdiffs
    SphP["EgyWtDensity"] = SphP["Density"]
    stop = False
    for _ in range(100):
        entropy(True)
        old = SphP["EgyWtDensity"].copy()
        density_call(ctx, pman, SphP, BhP, 0, 1)
        rounds += 1
        if stop:
            break
        gas = P["PI"][P["Type"] == 0]
        with np.errstate(invalid="ignore"):
            v = np.abs(SphP["EgyWtDensity"][gas] - old[gas]) / SphP["EgyWtDensity"][gas]
        maxdiffs.append(max(0.0, np.nanmax(v)))
        if maxdiffs[-1] < 1e-3:
            stop = True
    return first, rounds, maxdiffs


@pytest.mark.parametrize("disph", [0, 1])
def test_setup_smoothinglengths_equals_the_composition_of_its_pieces(ctx, disph):
    """The existing one-shot density is first called twice on one input.  It is bit-reproducible run to run here, so the comparison is
    by bytes; were it not, the 1e-10 relative bound of test_gpu_sph.py would apply (the branch below)."""
    sq.set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=0.5, DensityKernelType=1, BlackHoleNgbFactor=2.0, MinGasHsml=0.006)
    mean = cm.BOX / 16
    runs = []
    for _ in range(2):
        pman, SphP, BhP = st.hsml_set(16 ** 3)
        pman.Base["Hsml"] = mean
        density_call(ctx, pman, SphP, BhP, 1, 0)
        runs.append((pman.Base["Hsml"].copy(), SphP["Density"].copy()))
    reproducible = runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    print("one-shot density bit-reproducible run to run:", reproducible)

    pman, SphP, BhP = st.hsml_set(16 ** 3)
    wfirst, wrounds, wmaxdiffs = composed(ctx, pman, SphP, BhP, mean, disph)
    gman, gSphP, gBhP = st.hsml_set(16 ** 3)
    dp = cm.density_params(BoxSize=gman.BoxSize, BlackHoleOn=1)
    stats = sq.setup_smoothinglengths(ctx, -1, gman, gSphP, gBhP, dp, mean, U_INIT, ATIME, disph)
    print("setup_smoothinglengths disph=%d: %d rounds, maxdiff %s; first pass %d iterations; %d particles ended on the root"
          % (disph, stats.nrounds, list(stats.maxdiff), stats.first.niterations, stats.nbad_moments))
    assert stats.nrounds == wrounds and stats.first.niterations == wfirst.niterations and stats.first.ntargets == wfirst.ntargets
    assert (stats.nrounds >= 2) == bool(disph)
    pairs = [("Hsml", gman.Base["Hsml"], pman.Base["Hsml"]), ("DtHsml", gman.Base["DtHsml"], pman.Base["DtHsml"])]
    pairs += [(f, gSphP[f], SphP[f]) for f in ("Density", "EgyWtDensity", "DhsmlEgyDensityFactor", "DivVel", "CurlVel", "Entropy")]
    pairs += [("BH " + f, gBhP[f], BhP[f]) for f in ("Density", "DivVel")]
    pairs += [("maxdiff", np.array(stats.maxdiff), np.array(wmaxdiffs))]
    for name, got, want in pairs:
        if reproducible:
            assert got.tobytes() == want.tobytes(), name
        else:
            assert got.shape == want.shape and np.allclose(got, want, rtol=1e-10, atol=0, equal_nan=True), name
    # every other byte of the records is the caller's
    ref, _, _ = st.hsml_set(16 ** 3)
    for f in ref.Base.dtype.names:
        if f not in ("Hsml", "DtHsml"):
            assert gman.Base[f].tobytes() == ref.Base[f].tobytes(), f
    # no tree stays installed
    assert status_of(lambda: sq.tree_download(ctx, gman.NumPart, 0)) != 0


# ---- (5) the reference's own gates on the result --------------------------------------------------------------------------------------------

def test_setup_smoothinglengths_passes_the_reference_gates(ctx):
    """do_density_test's checks (tests/test_density.cpp:134-206) on the 32^3 grid of test_reference_gate_density_flat_gpu, and the
    relation the entropy loop converges to"""
    sq.set_densitypar(DensityResolutionEta=1.0, MaxNumNgbDeviation=0.5, DensityKernelType=1, BlackHoleNgbFactor=2.0, MinGasHsml=0.006)
    pos = cm.grid_positions(32)
    pman, SphP, BhP = cm.make_gas(pos, np.full(len(pos), 1.5 * cm.BOX / 32))
    BhP = np.zeros(2, dtype=sq.BH_SLOT_DTYPE)
    dp = cm.density_params(BoxSize=pman.BoxSize)
    stats = sq.setup_smoothinglengths(ctx, -1, pman, SphP, BhP, dp, cm.BOX / 32, U_INIT, ATIME, 1)
    P = pman.Base
    print("32^3 grid: mean Hsml %.6f, %d rounds, maxdiff %s" % (P["Hsml"].mean(), stats.nrounds, list(stats.maxdiff)))
    assert np.all(np.isfinite(P["Hsml"])) and np.all(SphP["Density"] > 0) and P["Hsml"].min() >= 0.006 and P["Hsml"].max() <= pman.BoxSize
    assert abs(P["Hsml"].mean() - 0.5) < 5e-4
    assert len(stats.maxdiff) >= 1 and stats.maxdiff[-1] < 1e-3 and stats.nrounds == len(stats.maxdiff) + 1
    g1 = st.GAMMA_MINUS1
    u = SphP["Entropy"] * np.power(SphP["EgyWtDensity"] / ATIME ** 3, g1) / g1
    err = np.abs(u / U_INIT - 1)
    bound = g1 * stats.maxdiff[-1] + 2 * POW4     # two pows, the device's and numpy's
    print("u from the final Entropy and EgyWtDensity: max relative error %.3g, bound %.3g" % (err.max(), bound))
    assert np.all(err <= bound)
    h0 = P["Hsml"].copy()
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    sq.density(ctx, None, 1, 0, 0, None, tree, pman, SphP, BhP)
    assert np.all(np.abs(h0 / P["Hsml"] - 1) < 0.5 / sq.GetNumNgb())


# ---- (6) early exits ----------------------------------------------------------------------------------------------------------------------

def test_setup_smoothinglengths_early_exits_leave_every_byte_alone(ctx):
    pman, SphP, BhP = st.hsml_set(64)
    before = (pman.Base.tobytes(), SphP.tobytes(), BhP.tobytes())
    dp = cm.density_params(BoxSize=pman.BoxSize, BlackHoleOn=1)
    assert sq.setup_smoothinglengths(ctx, 0, pman, SphP, BhP, dp, 0.5, U_INIT, ATIME, 1) is None
    assert (pman.Base.tobytes(), SphP.tobytes(), BhP.tobytes()) == before
    dm = cm.make_partmanager(cm.grid_positions(4))
    none = np.zeros(0, dtype=sq.SPH_DTYPE)
    before = dm.Base.tobytes()
    stats = sq.setup_smoothinglengths(ctx, -1, dm, none, None, dp, 0.5, U_INIT, ATIME, 1)
    assert dm.Base.tobytes() == before and stats.nrounds == 0 and stats.first.ntargets == 0
