"""Device time of the four parts of the routed black-hole step (shq_bh_accretion_marks / _marks_resolve / _feedback_effects /
_effects_apply) next to the one-shot shq_bh_accretion + shq_bh_feedback, in one context at tools/bench_subgrid.py's shape: n1^3 gas on
a jittered grid, nbh holes, every hole in the queue.  Times are the library's phase timers (HIP events on the context's stream, slots
15 / 17 / 18: walk + postprocess, count pass, route + sorts), medians over `reps` runs from the same starting state; the calls' wall
times (host marshalling, uploads, the host tree build of the routed calls) are printed beside them.  A report, not a gate: these
walks are latency-bound and the project claims no roofline for them.

usage: python tools/time_dist_bh.py [n1 = 128] [nbh = 5000] [reps = 5] [out = profiles/dist_bh_timing.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(len(os.sched_getaffinity(0))))
import shenqi_amd as sq  # noqa: E402
from shenqi_amd import capi  # noqa: E402
from shenqi_amd import dist as sd  # noqa: E402
from blackhole_fixtures import params as bh_params, make_work  # noqa: E402

n1 = int(sys.argv[1]) if len(sys.argv) > 1 else 128
nbh = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "dist_bh_timing.json")
BOX, TI = 8.0, 1 << 18
T_WALK, T_COUNT, T_ROUTE = 15, 17, 18
rng = np.random.default_rng(1)
ngas = n1 ** 3
sp = BOX / n1
g = np.arange(ngas)
gas = np.stack([g // n1 // n1, (g // n1) % n1, g % n1], axis=1) * sp
pos = np.concatenate([np.mod(gas + rng.normal(size=(ngas, 3)) * 0.25 * sp, BOX), rng.random((nbh, 3)) * BOX])
n = len(pos)
P0 = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
P0["Pos"] = pos
P0["Type"][ngas:] = 5
P0["Mass"] = 1.0
P0["ID"] = rng.permutation(n).astype(np.uint64) * 3 + 5
P0["Vel"] = rng.normal(size=(n, 3)) * 30
P0["FullTreeGravAccel"] = rng.normal(size=(n, 3)) * 50
P0["Hsml"] = sp * 1.6
P0["Hsml"][ngas:] = sp * 2.2
P0["TimeBinGravity"] = 20
P0["TimeBinHydro"] = 18
P0["PI"][:ngas] = np.arange(ngas)
P0["PI"][ngas:] = np.arange(nbh)
S0 = np.zeros(ngas, dtype=capi.SPH_DTYPE)
S0["Entropy"] = 100.0
S0["Density"] = ngas / BOX ** 3
B0 = np.zeros(nbh, dtype=capi.BH_DTYPE)
B0["Mass"] = 4.0
B0["Density"] = ngas / BOX ** 3
B0["Mtrack"] = 1.0
B0["CountProgs"] = 1
kf = sq.KickFactors()
for b in range(47):
    kf.gravkicks[b] = 1e-4
    kf.hydrokicks[b] = 1e-4
    kf.dloga_for_bin[b] = 1e-7 * 2.0 ** (b - 16) if b > 0 else 0.0
rnd = rng.random(8191)
cp, prm = bh_params(BoxSize=BOX)
queue = np.ascontiguousarray(np.arange(ngas, n, dtype=np.int32))
none = np.zeros(0, dtype=np.int32)
ctx = sq.Context(0)
rows = {}


def note(name, wall_ms, **slots):
    r = rows.setdefault(name, {"wall_ms": []})
    r["wall_ms"].append(wall_ms)
    for k, slot in slots.items():
        r.setdefault(k, []).append(ctx.timer_ms(slot))


def timed(name, fn, **slots):
    t0 = time.perf_counter()
    out = fn()
    note(name, (time.perf_counter() - t0) * 1e3, **slots)
    return out


def one_shot():
    pman = sd.records_pman(sq, BOX, P0)
    S, B = S0.copy(), B0.copy()
    ids = np.ascontiguousarray(pman.Base["ID"])
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK + sq.BHMASK)
    sq.force_tree_update_hmax(tree, pman)
    w, cw = make_work(ngas, nbh)
    pv, tv, sv, bv = pman.view(), tree.view(), capi.sph_view(S), capi.bh_slot_view(B)
    ns, nb = C.c_int64(), C.c_int64()
    timed("shq_bh_accretion", lambda: capi.check(capi.hip.shq_bh_accretion(
        ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(ids), capi.ptr(queue), len(queue), C.byref(kf), C.byref(cp), TI, capi.ptr(rnd), len(rnd),
        C.byref(cw))), walk_ms=T_WALK)
    timed("shq_bh_feedback", lambda: capi.check(capi.hip.shq_bh_feedback(
        ctx.h, C.byref(tv), C.byref(pv), C.byref(sv), C.byref(bv), capi.ptr(ids), capi.ptr(queue), len(queue), C.byref(kf), C.byref(cp), n + 100, capi.ptr(rnd), len(rnd),
        None, C.byref(cw), C.byref(ns), C.byref(nb))), walk_ms=T_WALK)
    return ns.value, nb.value, int((w["SPH_SwallowID"] != 0).sum())


ops = sd.GpuBhOps(ctx, BOX)          # one for all rounds: from the second on it offers the last count as the capacity, one count pass per walk


def in_parts():
    P, S, B = P0.copy(), S0.copy(), B0.copy()
    w = sd.bh_work_arrays(ngas, nbh)
    marks, _ = timed("shq_bh_accretion_marks", lambda: ops.accretion_marks(P, S, B, n, queue, none, none, 1, 0, 0, kf, prm, TI, rnd, w),
                     count_ms=T_COUNT, walk_ms=T_WALK, route_ms=T_ROUTE)
    timed("shq_bh_marks_resolve", lambda: ops.marks_resolve(P, marks, TI, ngas, nbh, w), walk_ms=T_WALK)
    effects, _ = timed("shq_bh_feedback_effects", lambda: ops.feedback_effects(P, S, B, n, queue, none, none, 1, 0, 0, kf, prm, rnd, w),
                       count_ms=T_COUNT, walk_ms=T_WALK, route_ms=T_ROUTE)
    res = timed("shq_bh_effects_apply", lambda: ops.effects_apply(P, S, B, effects, prm, n + 100, rnd, None, w), walk_ms=T_WALK)
    return res + (int((w["SPH_SwallowID"] != 0).sum()), len(marks), len(effects))


for r in range(reps + 1):
    a, b = one_shot(), in_parts()
    if a != b[:3]:                                            # the two routes should swallow the same and mark the same
        print("the routes differ: one-shot (gas, holes swallowed, gas marked) %s, in parts %s" % (a, b[:3]))
    if r == 0:                                                # the first round pays the first-use allocations
        rows.clear()
med = {name: {k: float(np.median(v)) for k, v in r.items()} for name, r in rows.items()}


def device(name):
    return sum(v for k, v in med[name].items() if k != "wall_ms")


one = device("shq_bh_accretion") + device("shq_bh_feedback")
parts = sum(device(k) for k in med if k not in ("shq_bh_accretion", "shq_bh_feedback"))
result = {"shape": {"gas": ngas, "holes": nbh, "box": BOX, "reps": reps}, "gas_swallowed": b[0], "holes_swallowed": b[1], "marks": b[3], "effects": b[4],
          "median_ms": med, "device_ms_one_shot_kernels": one, "device_ms_four_parts": parts, "ratio": parts / one,
          "note": "device_ms: phase timers (walk_ms: walk + postprocess, or sort + per-particle kernel; count_ms: the count pass, once per walk here since the "
                  "caller offered enough room, twice through the plain how-many-then-fill call; "
                  "route_ms: route kernel, two sorts, record write); wall_ms: the whole call from Python, host tree build of the routed walks included"}
for name, r in med.items():
    print("%-26s %s" % (name, "  ".join("%s %.3f" % kv for kv in r.items())))
print("device: one-shot kernels %.3f ms, four parts %.3f ms, ratio %.2f" % (one, parts, parts / one))
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
ctx.close()
