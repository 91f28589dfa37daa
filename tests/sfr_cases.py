"""Shared inputs of the star-formation tests (test_sfr_cpu.py, test_gpu_sfr.py): the cooling random case's parameters (Sherwood / Verner96,
self-shielding, the global UVB at z = 3), the reference's default star-formation parameters, a dense particle set with named edge rows,
and the restatement's and the host engine's results over them.  Everything is computed once and handed out read-only."""
import functools
import math

import numpy as np

import shenqi_amd as sq
from shenqi_amd import capi
import cooling_restated as cr
import cooling_cases as cc
import sfr_restated as sr

# The seed was chosen on the CPU, the smallest from 20261018 on with which the host engine and a second host build with SHQ_COOL_NUDGE
# (every log / exp / pow / log10 result moved by one ulp in alternating sign) agree in EVERY discrete outcome of EVERY particle of the
# set below, edge rows included, under each BHFeedbackUseTcool 0..3: the decision code, the fourth clause of sfreff_on_eeqos, the
# tcool < trelax branch, egycurrent > egyeff (both in the branch byte) and the status.  test_sfr_cpu.py recomputes this agreement and
# the smallest margins, which are recorded there.
SEED = 20261018
NDENSE = 2048 + 37
NRND = 4096
REDSHIFT = 3.0
A3INV = (1 + REDSHIFT) ** 3
HUBBLE = 0.1 * math.sqrt(0.3 * A3INV + 0.7)          # internal units, Omega0 = 0.3, flat
AVG_BARYON_MASS = 0.0035
DLOGA_FOR_BIN = {0: 1e-3, 20: 0.0, 22: 2.5e-4, 24: 1e-3, 26: 4e-3}       # bin 0 (no relaxation) and a bin with dloga = 0
EDGE_ROWS = ("tsfr_below_dtime", "deferred_bh_heated", "in_the_wind", "below_overdensity")
CRITERIA = (1, 3, 5, 13, 21, 3 | 5)


def _ro(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def case():
    return cc.random_case()[0]


def params(**kw):
    """the reference-default parameter set as the restatement's dict"""
    kw.setdefault("avg_baryon_mass", AVG_BARYON_MASS)
    return sr.default_params(case().units, **kw)


def lib_params(par):
    return sq.sfr_params(**{k: v for k, v in par.items() if k != "StarformationOn"})


@functools.lru_cache(maxsize=None)
def rnd_table(seed=SEED):
    t = np.random.default_rng(seed + 1).random(NRND)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def particles(seed=SEED):
    """the dense set followed by the edge rows (EDGE_ROWS, in that order)"""
    par = params()
    rng = np.random.default_rng(seed)
    n = NDENSE
    phys = par["PhysDensThresh"] * 10.0 ** rng.uniform(0, 4, n)
    dens = phys / A3INV
    u = 10.0 ** rng.uniform(math.log10(par["EgySpecCold"]), 7, n)
    enttou = np.array([cr.entropy_to_u(float(d), A3INV) for d in dens])
    ne = rng.uniform(0, 1.2, n)
    ne[rng.random(n) < 0.05] = 0.0
    bins = np.array(sorted(DLOGA_FOR_BIN))[rng.integers(0, len(DLOGA_FOR_BIN), n)]
    flags = ((rng.integers(0, 4, n) << 4) | (8 * (rng.random(n) < 0.3)) | (4 * (rng.random(n) < 0.5))).astype(np.uint8)
    p = dict(Density=dens, Entropy=u / enttou, Ne=ne, Metallicity=rng.uniform(0, 0.05, n), Mass=AVG_BARYON_MASS * rng.uniform(0.4, 2.5, n),
             Hsml=rng.uniform(0.5, 5.0, n), DivVel=rng.normal(0, 300, n), CurlVel=np.abs(rng.normal(0, 300, n)), GradRho=dens * 10.0 ** rng.uniform(-2, 1, n),
             dloga=np.array([DLOGA_FOR_BIN[int(b)] for b in bins]), DelayTime=np.zeros(n), timebin=bins.astype(np.uint8), flags=flags,
             ID=rng.integers(1, 2 ** 56, n, dtype=np.uint64))
    p["Metallicity"][rng.random(n) < 0.05] = 0.0
    p["GradRho"][rng.random(n) < 0.05] = 0.0

    thr = par["PhysDensThresh"] / A3INV

    def row(density, u, **kw):
        r = {k: v[7] for k, v in p.items()}     # an ordinary particle of the set with its density, energy and time step set
        r.update(Density=density, Entropy=u / cr.entropy_to_u(density, A3INV), timebin=24, dloga=DLOGA_FOR_BIN[24], flags=np.uint8(0), DelayTime=0.0)
        r.update(kw)
        return r

    edge = [row(1e4 * thr, 2e3, dloga=0.05),                    # tsfr = 0.015 < dtime = 0.11
            row(10 * thr, 5e7, flags=np.uint8(8)),              # BHHeated, egycurrent ~2.4e9 K, off the rate table: DEFERRED in cooling_relaxed
            row(10 * thr, 2e3, DelayTime=0.3),
            row(0.5 * par["OverDensThresh"], 2e3)]
    assert len(edge) == len(EDGE_ROWS)
    for k in p:
        p[k] = np.concatenate([p[k], np.array([e[k] for e in edge], dtype=p[k].dtype)])
    return _ro(p)


def heating_uvbg():
    """a synthetic strong-heating UVBG: the global one with photoheating far above any cooling, so that GetCoolingTime returns 0"""
    uv = dict(case().uv)
    uv.update(epsH0=1e-8, epsHe0=1e-8, epsHep=1e-8)
    return uv


def subset(p, idx):
    return {k: v[idx] for k, v in p.items()}


def _part(p, k):
    return dict(Density=float(p["Density"][k]), Entropy=float(p["Entropy"][k]), Ne=float(p["Ne"][k]), Metallicity=float(p["Metallicity"][k]), Sfr=0.0,
                DelayTime=float(p["DelayTime"][k]), Mass=float(p["Mass"][k]), Hsml=float(p["Hsml"][k]), ID=int(p["ID"][k]), TimeBinHydro=int(p["timebin"][k]),
                flags=int(p["flags"][k]), dloga=float(p["dloga"][k]), DivVel=float(p["DivVel"][k]), CurlVel=float(p["CurlVel"][k]), GradRho=float(p["GradRho"][k]))


def restated(what, par, p, local_uv=None):
    """the restatement over arrays, in the library's layout: (out [NOUT][n], flags, decision, branch, evaluations, left the table)"""
    c = case()
    S = sr.Sfr(c.cool, par, REDSHIFT, A3INV, HUBBLE, c.uv, c.uv if local_uv is None else local_uv, rnd_table())
    n = len(p["Density"])
    out = np.zeros((len(capi.SFR_OUT), n))
    flags, decision, branch = (np.zeros(n, dtype=np.uint8) for _ in range(3))
    ev, left = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    for k in range(n):
        r, ev[k], left[k] = S.run(what, _part(p, k))
        for i, name in enumerate(capi.SFR_OUT):
            out[i, k] = r.get(name, 0.0)
        flags[k], decision[k], branch[k] = r["flags"], r["decision"], r["branch"]
    return out, flags, decision, branch, ev, left


def host(what, par, p, local_uv=None, nthreads=0, entry=None):
    """shq_sfr_eval_host; entry: that function of another build of the host engine (build_nudged), driven through the same wrapper"""
    c = case()
    local = None if local_uv is None else c.uvbg(local_uv)
    if entry is None:
        return sq.sfr_eval_host(c.tables(), lib_params(par), what, p, c.uvbg(), REDSHIFT, A3INV, HUBBLE, rnd_table(), uvbg_local=local, nthreads=nthreads)
    import ctypes as C
    tables = c.tables()
    return sq._sfr_eval(entry, C.byref(tables), lib_params(par), what, p, c.uvbg(), local, REDSHIFT, A3INV, HUBBLE, rnd_table(), (int(nthreads),))


def heating_subset():
    """the first 256 particles and the edge rows: what the net-heating runs go over"""
    n = len(particles()["Density"])
    return subset(particles(), np.r_[0:256, n - len(EDGE_ROWS):n])


@functools.lru_cache(maxsize=None)
def host_starform(tcool=1):
    """shq_sfr_eval_host STARFORM on the whole set with the default parameters, once"""
    r = host("STARFORM", params(BHFeedbackUseTcool=tcool), particles())
    for a in r.arrays():
        a.setflags(write=False)
    return r


def dump_sets():
    """(what, parameters, local UVBG or None for the global one) of the runs a dump holds; the last three are the net-heating rows"""
    hot = heating_uvbg()
    return [("STARFORM", params(BHFeedbackUseTcool=t), None) for t in range(4)] + \
           [("STARFORM", params(StarformationCriterion=3 | 21), None), ("NH0", params(BHFeedbackUseTcool=2), None), ("STARFORM", params(QuickLymanAlphaProbability=0.5), None)] + \
           [("STARFORM", params(BHFeedbackUseTcool=t), hot) for t in (1, 3)] + [("NH0", params(), hot)]


def dump(path):
    """the whole set, the tables and the host engine's results as one binary file for tools/sfr_host_main.cpp"""
    c, p, sets = case(), particles(), dump_sets()
    n = len(p["Density"])
    st = capi.SfrEvalStep(REDSHIFT, A3INV, HUBBLE, c.uvbg(), c.uvbg(), None, NRND)
    with open(path, "wb") as f:
        f.write(np.array([n, NRND, len(sets)], dtype=np.int64).tobytes())
        t = c.tables()
        rates = np.ascontiguousarray(c.net.tab, dtype=np.float64)
        t.rate_tables = None
        f.write(bytes(t))
        f.write(rates.tobytes())
        f.write(bytes(st))
        f.write(rnd_table().tobytes())
        for k in capi.SFR_ARRAYS:
            f.write(np.ascontiguousarray(p[k]).tobytes())
        for what, par, local in sets:
            r = host(what, par, p, local_uv=local)
            f.write(bytes(lib_params(par)))
            f.write(bytes(c.uvbg(local)))
            f.write(np.int32(capi.SFR_WHAT[what]).tobytes())
            for a in (r.out, r.flags, r.decision, r.branch, r.status, r.steps):
                f.write(np.ascontiguousarray(a).tobytes())


def build_nudged(workdir):
    """the second host build: cooling_host.hip and sfr_host.hip with SHQ_COOL_NUDGE, host code only; returns its shq_sfr_eval_host
    and the header's sizes of shq_sfr_params, shq_sfr_arrays, shq_sfr_eval_step, shq_sfr_fields and shq_sfr_result as that compiler sees them"""
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(str(workdir), "libsfr_nudged.so")
    src = [os.path.join(root, "shenqi_amd", "csrc", "cooling_host.hip"), os.path.join(root, "shenqi_amd", "csrc", "sfr_host.hip"), os.path.join(root, "tests", "sfr_host_shim.cpp")]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-fPIC", "-shared", "-DSHQ_COOL_NUDGE",
                           "-I" + os.path.join(root, "include")] + src + ["-o", lib, "-lpthread"])
    dll = C.CDLL(lib)
    entry = dll.shq_sfr_eval_host
    entry.argtypes, entry.restype = capi.hip.shq_sfr_eval_host.argtypes, C.c_int
    sizes = (C.c_int64 * 5)()
    dll.shq_sfr_struct_sizes(sizes)
    return entry, list(sizes)


def margins(r, p):
    """how far each particle of a STARFORM result is from each libm-dependent discrete decision, relative: the smallest per decision"""
    ok = r.status == capi.COOL_OK
    b = r.branch
    with np.errstate(all="ignore"):
        draw = rnd_table()[((np.asarray(p["ID"]) + np.uint64(1)) % np.uint64(NRND)).astype(np.int64)]
        sel = ok & (r.prob > 0)
        m = {"draw": np.min(np.abs(draw[sel] - r.prob[sel]) / r.prob[sel])}
        sel = ok & ((b & capi.SFR_B_CLAUSE4) != 0)
        if sel.any():
            unew = np.asarray(p["Entropy"])[sel] * np.array([cr.entropy_to_u(float(d), A3INV) for d in np.asarray(p["Density"])[sel]])
            m["clause4"] = np.min(np.abs(unew - 3.2 * r.egyeff4[sel]) / (3.2 * r.egyeff4[sel]))
        sel = ok & ((b & capi.SFR_B_TCOOL) != 0) & (r.tcool_relax > 0)
        if sel.any():
            m["tcool_vs_trelax"] = np.min(np.abs(r.tcool_relax[sel] - r.trelax[sel]) / r.trelax[sel])
        sel = ok & ((b & capi.SFR_B_RELAXED) != 0)
        if sel.any():
            m["egycurrent_vs_egyeff"] = np.min(np.abs(r.egycurrent[sel] - r.egyeff[sel]) / r.egyeff[sel])
            m["egycurrent_vs_5e6"] = np.min(np.abs(r.egycurrent[sel] - 5e6) / 5e6)
    return {k: float(v) for k, v in m.items()}
