"""Brute-force numpy restatements of the four parts of the sharded black-hole step (shq_bh_accretion_marks / _marks_resolve /
_feedback_effects / _effects_apply), the set builder of its tests and the comparison with the undivided run.  TEST INFRASTRUCTURE ONLY.

The arithmetic is oracle/blackhole.py's, expression by expression: `accretion_marks` and `feedback_effects` are its two loops with
every write on the neighbours' side turned into a record, `marks_resolve` and `effects_apply` do those writes per particle in
ascending hole order.  The yardstick of the tests is oracle/blackhole.py itself (accretion + feedback) on the undivided set with the
global queue: its loops run in queue order, which is the order the owners apply in."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import blackhole as obh  # noqa: E402
from blackhole import GAMMA_MINUS1, TIMEBINS, dm_velpred, is_timebin_active, kernel_wk, neighbours, sph_velpred  # noqa: E402

NMESH = 48
TI = 1 << 18                     # bins 16..18 active, 19 and 20 not
# the three parameter sets of tests/test_gpu_blackhole.py: (seed, queue stride, parameters)
CASES = {"thermal": (3, 1, {}),
         "bound": (4, 2, dict(RepositionEnabled=0, MergeGravBound=1, SeedBHDynMass=2.0, BH_DRAG=1, WindsDecoupleSph=1, DensityKernelType=4)),
         "kinetic": (5, 1, dict(BlackHoleKineticOn=1, DensityKernelType=2))}
FACES = (4.0, 8.0 / 3)           # slab faces of two and of three equal x-slabs of the box of 8


def _records(out, dtype, nranks):
    rec = np.array(out, dtype=dtype) if out else np.zeros(0, dtype=dtype)
    rec = rec[np.lexsort((rec["hole"], rec["part_index"], rec["owner"]))]
    return rec, np.bincount(rec["owner"], minlength=nranks).astype(np.int64)


def _router(nlocal, gown, gidx, rank):
    def route(other):
        return (rank, int(other)) if other < nlocal else (int(gown[other - nlocal]), int(gidx[other - nlocal]))
    return route


def accretion_marks(P, S, B, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, Ti_Current, rnd, work):
    """oracle/blackhole.py:accretion without the two mark arrays: a record where it would have marked"""
    from shenqi_amd import capi
    ids, kt, route, out = P["ID"], prm.DensityKernelType, _router(nlocal, gown, gidx, rank), []
    for t, i in enumerate(queue):
        pi = int(P["PI"][i])
        H = float(P["Hsml"][i])
        myid = int(ids[i])
        Ivel = P["Vel"][i].copy()
        Iacc = P["FullTreeGravAccel"][i] + P["GravPM"][i] + B["DFAccel"][pi]
        Imass, Ibh, Idens, Imtrack = float(P["Mass"][i]), float(B["Mass"][pi]), float(B["Density"][pi]), float(B["Mtrack"][pi])
        enc, fws, sment, gv, mgas = 0, 0.0, 0.0, np.zeros(3), 0.0
        idx, r2s, ds = neighbours(P, i, prm.BoxSize)
        for other, r2, dx in zip(idx, r2s, ds):
            other = int(other)
            r = np.sqrt(r2)
            if P["Mass"][other] < 0:
                continue
            ty = int(P["Type"][other])
            if prm.WindsDecoupleSph and ty == 0 and S["DelayTime"][P["PI"][other]] > 0:
                continue
            if int(ids[other]) == myid:
                continue
            if ty == 5 and r < (2 * prm.ForceSoftening / 2.8):
                enc = 1
                flag = 0
                if prm.RepositionEnabled == 1:
                    flag = 1
                if prm.MergeGravBound == 0:
                    flag = 1
                opi = int(P["PI"][other])
                if prm.MergeGravBound == 1 and prm.RepositionEnabled == 0:
                    vp = dm_velpred(P, other, kf)
                    KE = PE = 0.0
                    for d in range(3):
                        dv = Ivel[d] - vp[d]
                        da = Iacc[d] - P["FullTreeGravAccel"][other][d] - P["GravPM"][other][d] - B["DFAccel"][opi][d]
                        KE += 0.5 * (dv * dv)
                        PE += da * dx[d]
                    KE /= (prm.atime * prm.atime)
                    PE /= prm.atime
                    flag = 1 if PE + KE <= 0 else 0
                if flag == 1:
                    out.append(route(other) + (off + t, 0, myid))
            if ty == 0 and r2 < H * H:
                u = r * (1.0 / H)
                wk = kernel_wk(u, H, kt)
                mj = float(P["Mass"][other])
                spi = int(P["PI"][other])
                sment += (mj * wk * S["Entropy"][spi])
                vp = sph_velpred(P, S, other, kf)
                gv += mj * wk * vp
                p = 0.0
                part = Imass
                if prm.SeedBHDynMass > 0 and Imtrack < prm.SeedBHDynMass:
                    part = Imtrack
                if (Ibh - part) > 0 and Idens > 0:
                    p = (Ibh - part) * wk / Idens
                if rnd[int(ids[other]) % len(rnd)] < p:
                    out.append(route(other) + (off + t, 1, myid))
                fws += (mj * wk)
                if prm.BlackHoleKineticOn == 1:
                    mgas += mj
        B["encounter"][pi] = enc
        work["BH_FeedbackWeightSum"][pi] = fws
        work["BH_Entropy"][pi] = sment
        work["BH_SurroundingGasVel"][pi] = gv
        work["MgasEnc"][pi] = mgas
    for i in queue:
        obh.accretion_postprocess(P, B, int(i), kf, prm, work)
    return _records(out, capi.BH_MARK_DTYPE, nranks)


def marks_resolve(P, marks, Ti_Current, nsph, nbh, work):
    """the two mark rules (oracle/blackhole.py:125-129 and :145-146), a particle's marks in ascending hole order"""
    work["SPH_SwallowID"][:nsph] = 0
    work["BH_SwallowID"][:nbh] = 0
    for k in np.lexsort((marks["hole"], marks["part_index"])):
        other, myid = int(marks["part_index"][k]), int(marks["id"][k])
        opi = int(P["PI"][other])
        if marks["kind"][k] == 1:
            assert P["Type"][other] == 0
            if int(work["SPH_SwallowID"][opi]) < myid + 1:
                work["SPH_SwallowID"][opi] = myid + 1
            continue
        assert P["Type"][other] == 5
        readid = int(work["BH_SwallowID"][opi])
        if readid != 0 and readid < myid:
            work["BH_SwallowID"][opi] = myid + 1
        elif readid == 0 and (int(P["ID"][other]) < myid or not is_timebin_active(P["TimeBinHydro"][other], Ti_Current)):
            work["BH_SwallowID"][opi] = myid + 1


def feedback_effects(P, S, B, nlocal, queue, gown, gidx, nranks, rank, off, kf, prm, rnd, work):
    """oracle/blackhole.py:feedback with nothing written on the neighbours' side: a record per swallow, heat and kick"""
    from shenqi_amd import capi
    ids, kt, route, out = P["ID"], prm.DensityKernelType, _router(nlocal, gown, gidx, rank), []
    todo = [(t, int(i)) for t, i in enumerate(queue) if work["BH_SwallowID"][P["PI"][i]] == 0]
    for t, i in todo:
        pi = int(P["PI"][i])
        H = float(P["Hsml"][i])
        myid = int(ids[i])
        Idens, Imtrack = float(B["Density"][pi]), float(B["Mtrack"][pi])
        fws = float(work["BH_FeedbackWeightSum"][pi])
        dtime = kf.dloga_for_bin[int(P["TimeBinHydro"][i])] / prm.hubble
        fbe = prm.BlackHoleFeedbackFactor * 0.1 * B["Mdot"][pi] * dtime * prm.LightOverUnitVel ** 2
        channel, kefb = 0, 0.0
        if prm.BlackHoleKineticOn == 1 and work["KEflag"][pi] > 0:
            channel = 1
            if work["KEflag"][pi] == 2:
                kefb = float(B["KineticFdbkEnergy"][pi])
        accm, accbh, mom, cprog, mintb = 0.0, 0.0, np.zeros(3), 0, TIMEBINS
        idx, r2s, _ = neighbours(P, i, prm.BoxSize)
        for other, r2 in zip(idx, r2s):
            other = int(other)
            ty = int(P["Type"][other])
            if int(ids[other]) == myid:
                continue
            if prm.WindsDecoupleSph and ty == 0 and S["DelayTime"][P["PI"][other]] > 0:
                continue
            opi = int(P["PI"][other])
            if ty == 5 and work["BH_SwallowID"][opi] != 0:
                if int(work["BH_SwallowID"][opi]) != myid + 1:
                    continue
                out.append(route(other) + (off + t, 0, 0.0))
                cprog += int(B["CountProgs"][opi])
                accbh += float(B["Mass"][opi])
                om = float(P["Mass"][other])
                if prm.SeedBHDynMass > 0 and Imtrack > 0:
                    if B["Mtrack"][opi] < prm.SeedBHDynMass:
                        om = float(B["Mtrack"][opi])
                accm += om
                mom += om * dm_velpred(P, other, kf)
            if ty == 0 and work["SPH_SwallowID"][opi] == 0 and r2 < H * H:
                if mintb > P["TimeBinHydro"][other]:
                    mintb = int(P["TimeBinHydro"][other])
                u = np.sqrt(r2) * (1.0 / H)
                mj = float(P["Mass"][other])
                wk = kernel_wk(u, H, kt)
                if fws > 0 and fbe > 0 and channel == 0 and mj > 0:
                    inj = fbe * mj * wk / fws
                    out.append(route(other) + (off + t, 2, inj / mj))
                if kefb > 0 and channel == 1 and Idens > 0:
                    out.append(route(other) + (off + t, 3, np.sqrt(2 * kefb * wk / Idens)))
            if ty == 0 and int(work["SPH_SwallowID"][opi]) == myid + 1:
                mj = float(P["Mass"][other])
                accm += mj
                mom += mj * sph_velpred(P, S, other, kf)
                out.append(route(other) + (off + t, 1, 0.0))
        work["BH_accreted_Mass"][pi] = accm
        work["BH_accreted_BHMass"][pi] = accbh
        work["BH_accreted_momentum"][pi] = mom
        B["minTimeBin"][pi] = mintb
        B["CountProgs"][pi] += cprog
    for _, i in todo:                                       # blackhole_feedback_postprocess, oracle/blackhole.py:294-312
        pi = int(P["PI"][i])
        if work["BH_accreted_BHMass"][pi] > 0:
            B["Mass"][pi] += work["BH_accreted_BHMass"][pi]
        if work["BH_accreted_Mass"][pi] > 0:
            accmass = float(work["BH_accreted_Mass"][pi])
            pm = np.float32(P["Mass"][i])
            for k in range(3):
                P["Vel"][i][k] = (P["Vel"][i][k] * float(pm) + work["BH_accreted_momentum"][pi][k]) / (float(pm) + accmass)
            sd = prm.SeedBHDynMass
            if sd > 0 and B["Mtrack"][pi] + accmass < sd:
                B["Mtrack"][pi] += accmass
            elif B["Mtrack"][pi] < sd:
                P["Mass"][i] = np.float32(B["Mtrack"][pi] + accmass)
                B["Mtrack"][pi] = sd
            else:
                P["Mass"][i] = np.float32(float(pm) + accmass)
        if prm.BlackHoleKineticOn == 1 and work["KEflag"][pi] == 2:
            B["KineticFdbkEnergy"][pi] = 0
    return _records(out, capi.BH_EFFECT_DTYPE, nranks)


def effects_apply(P, S, B, effects, prm, maxpart, rnd, eeqos, work):
    """the neighbours' side of oracle/blackhole.py:feedback, a particle's records in ascending hole order"""
    nsph = nbh = 0
    for k in np.lexsort((effects["hole"], effects["part_index"])):
        other, kind, value = int(effects["part_index"][k]), int(effects["kind"][k]), float(effects["value"][k])
        opi = int(P["PI"][other])
        assert P["Type"][other] == (5 if kind == 0 else 0)
        if kind == 0:
            nbh += int((P["Flags"][other] & 2) == 0)
            B["SwallowID"][opi] = int(work["BH_SwallowID"][opi]) - 1
            B["SwallowTime"][opi] = prm.atime
            P["Flags"][other] |= 2
            B["encounter"][opi] = 0
        elif kind == 1:
            nsph += int((P["Flags"][other] & 1) == 0)
            P["Flags"][other] |= 1
            S["ReverseLink"][opi] = maxpart + 100
        elif kind == 2:
            if eeqos is not None and eeqos[other]:
                P["Flags"][other] |= 8
            enttou = (S["Density"][opi] * prm.a3inv) ** GAMMA_MINUS1 / GAMMA_MINUS1
            unew = S["Entropy"][opi] * enttou
            unew += value
            if unew > prm.MaxThermalU:
                unew = prm.MaxThermalU
            S["Entropy"][opi] = unew / enttou
        else:
            idn = int(P["ID"][other])
            theta = np.arccos(2 * rnd[(idn + 3) % len(rnd)] - 1)
            phi = 2 * np.pi * rnd[(idn + 4) % len(rnd)]
            direc = np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])
            P["Vel"][other] += value * direc
    return nsph, nbh


class RestatedBhOps:
    """DistBlackHole's operators on the CPU; keeps the lists it received for what the tests assert about their own inputs"""

    def __init__(self):
        self.marks = self.effects = None

    def accretion_marks(self, *a):
        return accretion_marks(*a)

    def marks_resolve(self, P, marks, *a):
        self.marks = marks.copy()
        return marks_resolve(P, marks, *a)

    def feedback_effects(self, *a):
        return feedback_effects(*a)

    def effects_apply(self, P, S, B, effects, *a):
        self.effects = effects.copy()
        return effects_apply(P, S, B, effects, *a)


# ---- the set ----------------------------------------------------------------------------------------------------------------------
def place_holes(P, bi, stride, rng):
    """blackhole_fixtures.setup scatters its merging pairs at random: about one in sixty would lie across a slab face.  Here eight
    pairs and the chain of three straddle a face by 0.08 (the merging radius is 0.25): pair j at FACES[(j // 2) % 2] with its larger
    ID left of the face for even j, right for odd j; both members are in a queue of every stride-th hole.  The chain a - mid - b lies
    across FACES[0] with a on the left.  Pairs 0 to 3 are bound: setup's rule for the moved positions,
    ten times as strong, since a hole may carry the pull setup gave it towards its former partner, and both
    in active time bins: two inactive holes mark each other, and then neither swallows."""
    box = 8.0
    for j in range(8):
        a, b = int(bi[2 * stride * j]), int(bi[2 * stride * j + stride])
        if (P["ID"][a] > P["ID"][b]) != (j % 2 == 0):
            a, b = b, a
        y, z = rng.random(2) * box
        P["Pos"][a] = [FACES[(j // 2) % 2] - 0.04, y, z]
        P["Pos"][b] = [FACES[(j // 2) % 2] + 0.04, y + 0.01, z - 0.01]
        if j < 4:
            P["TimeBinHydro"][a], P["TimeBinHydro"][b] = 17, 18
            P["Vel"][b] = P["Vel"][a] + 0.01
            P["FullTreeGravAccel"][b] = P["FullTreeGravAccel"][a] + 50000.0 * obh.nearest(P["Pos"][a] - P["Pos"][b], box)
    a, mid, b = int(bi[16 * stride]), int(bi[16 * stride + 2]), int(bi[16 * stride + 1])
    y, z = rng.random(2) * box
    P["Pos"][a], P["Pos"][mid], P["Pos"][b] = [FACES[0] - 0.07, y, z], [FACES[0] + 0.01, y, z], [FACES[0] + 0.09, y, z]


def global_set(case, bh_hsml=1.0, size=None, place=True):
    """(P, S, B, kf, rnd, queue, prm, eeqos, MaxPart) of a parameter set: blackhole_fixtures.setup with the holes placed on purpose"""
    from blackhole_fixtures import params, setup
    seed, stride, kw = CASES[case]
    _, prm = params(**kw)
    pman, S, B, kf, rnd, bi = setup(seed, bh_hsml=bh_hsml, **(size or {}))
    P = pman.Base.copy()
    if place:
        place_holes(P, bi, stride, np.random.default_rng(100 + seed))
    queue = np.ascontiguousarray(bi[::stride].astype(np.int32))
    return P, S, B, kf, rnd, queue, prm, (np.arange(len(P)) % 3 == 0).astype(np.uint8), len(P) + 50


def owners(decomp, P):
    return decomp.owner_of(torch.from_numpy(np.ascontiguousarray(P["Pos"][:, 0]))).numpy()


def decomp_of(world):
    import common as cm
    from shenqi_amd import dist as sd

    class FakeComm:
        size, rank = world, 0
    return sd.SlabDecomp(FakeComm(), NMESH, cm.BOX)


def global_order(decomp, Pg, queueg, nranks, empty=()):
    """positions in queueg of the global queue the sharded run applies: the ranks' queues one after the other, in rank order"""
    own = owners(decomp, Pg)[queueg]
    return np.concatenate([np.flatnonzero(own == r) if r not in empty else np.zeros(0, dtype=np.int64) for r in range(nranks)]).astype(np.int64)


def local_part(rank, decomp, Pg, Sg, Bg, queueg, keep_queue=True):
    """this rank's share: its particles with their slots renumbered locally, the holes of the global queue it owns in that queue's order"""
    mine = np.flatnonzero(owners(decomp, Pg) == rank)
    P = Pg[mine].copy()
    gas, hole = P["Type"] == 0, P["Type"] == 5
    S, B = Sg[P["PI"][gas]].copy(), Bg[P["PI"][hole]].copy()
    P["PI"][gas] = np.arange(gas.sum())
    P["PI"][hole] = np.arange(hole.sum())
    back = {int(g): k for k, g in enumerate(mine)}
    queue = np.array([back[int(g)] for g in queueg if int(g) in back] if keep_queue else [], dtype=np.int32)
    return P, S, B, queue, mine


def reference(case, world, empty=(), **kw):
    """oracle/blackhole.py on the undivided set, its queue in the order the sharded run applies: dict of P, S, B, work, counts"""
    from blackhole_fixtures import make_work
    Pg, Sg, Bg, kf, rnd, queueg, prm, eeqos, maxpart = global_set(case, **kw)
    queue = queueg[global_order(decomp_of(world), Pg, queueg, world, empty)]
    P, S, B = Pg.copy(), Sg.copy(), Bg.copy()
    work, _ = make_work(len(S), len(B))
    counts = (0, 0)
    if len(queue):
        obh.accretion(P, S, B, P["ID"], queue, kf, prm, TI, rnd, work)
        acc_mass = B["Mass"].copy()
        counts = obh.feedback(P, S, B, P["ID"], queue, kf, prm, maxpart, rnd, eeqos, work)
    else:
        work["SPH_SwallowID"][:] = 0
        work["BH_SwallowID"][:] = 0
        acc_mass = B["Mass"].copy()
    return dict(P=P, S=S, B=B, work=work, counts=counts, queue=queue, Pg=Pg, Sg=Sg, Bg=Bg, acc_mass=acc_mass, prm=prm)


def run_rank(comm, rank, ops, case, empty=(), **kw):
    """one rank of DistBlackHole.run on global_set(case); ranks in `empty` run with an empty queue"""
    from shenqi_amd import dist as sd
    Pg, Sg, Bg, kf, rnd, queueg, prm, eeqos, maxpart = global_set(case, **kw)
    import common as cm
    decomp = sd.SlabDecomp(comm, NMESH, cm.BOX)
    P, S, B, queue, mine = local_part(rank, decomp, Pg, Sg, Bg, queueg, keep_queue=rank not in empty)
    drv = sd.DistBlackHole(comm, decomp, ops)
    counts = drv.run(P, S, B, queue, kf, prm, TI, maxpart, rnd, eeqos[mine])
    return dict(rows=mine, P=P, S=S, B=B, work=drv.work, counts=counts, nq=len(queue), nghost=drv.nghost, marks_sent=list(drv.marks_sent),
                effects_sent=list(drv.effects_sent), marks=getattr(ops, "marks", None), effects=getattr(ops, "effects", None))


P_EXACT, P_FLOAT = ("Flags", "Type"), ("Vel",)
S_EXACT, S_FLOAT = ("ReverseLink",), ("Entropy",)
B_EXACT = ("SwallowID", "encounter", "CountProgs", "minTimeBin")
B_FLOAT = ("Mass", "Mtrack", "SwallowTime", "KineticFdbkEnergy", "Mdot", "DragAccel")
W_EXACT = ("SPH_SwallowID", "BH_SwallowID", "KEflag")
W_FLOAT = ("BH_FeedbackWeightSum", "BH_Entropy", "BH_SurroundingGasVel", "MgasEnc", "BH_accreted_Mass", "BH_accreted_BHMass", "BH_accreted_momentum")


def assemble(results, ref):
    """the ranks' results put back into the undivided set's rows and slots: dict of P, S, B, work, counts"""
    Pg = ref["Pg"]
    P, S, B = Pg.copy(), ref["Sg"].copy(), ref["Bg"].copy()
    work = {k: np.zeros_like(v) for k, v in ref["work"].items()}
    seen, counts = 0, np.zeros(2, dtype=np.int64)
    for r in results:
        rows, lp = r["rows"], r["P"]
        seen += len(rows)
        for k in P_EXACT + P_FLOAT + ("Mass",):
            P[k][rows] = lp[k]
        gas, hole = lp["Type"] == 0, lp["Type"] == 5
        S[Pg["PI"][rows[gas]]] = r["S"][lp["PI"][gas]]
        B[Pg["PI"][rows[hole]]] = r["B"][lp["PI"][hole]]
        for k, v in r["work"].items():
            sel = gas if k == "SPH_SwallowID" else hole
            work[k][Pg["PI"][rows[sel]]] = v[lp["PI"][sel]]
        counts += r["counts"]
    assert seen == len(Pg)
    return dict(P=P, S=S, B=B, work=work, counts=tuple(int(c) for c in counts))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max(initial=0.0) / max(np.abs(b).max(initial=0.0), 1e-300))


def compare(got, ref, slot_tol=1e-12, work_tol=1e-11, mass_tol=1e-7):
    """integers equal; floats within the bars tests/test_gpu_blackhole.py uses against the same restatement (slot fields, Entropy and Vel
    1e-12, work sums 1e-11, the float particle mass 1e-7), relative to the field's largest value.  Returns the largest differences."""
    assert got["counts"] == tuple(ref["counts"])
    for rec, names in (("P", P_EXACT), ("S", S_EXACT), ("B", B_EXACT), ("work", W_EXACT)):
        for k in names:
            assert np.array_equal(got[rec][k], ref[rec][k]), (rec, k)
    worst = {}
    for rec, names, tol in (("P", P_FLOAT, slot_tol), ("S", S_FLOAT, slot_tol), ("B", B_FLOAT, slot_tol), ("work", W_FLOAT, work_tol), ("P", ("Mass",), mass_tol)):
        for k in names:
            worst[k] = rel(got[rec][k], ref[rec][k])
            assert worst[k] <= tol, (rec, k, worst[k], tol)
    return worst


# ---- what the set has to hold with two x-slabs --------------------------------------------------------------------------------------
def straddle_conditions(ref, results):
    """Asserted on the undivided restatement and on what two ranks received: see tests/test_dist_bh_cpu.py.  Returns the counts."""
    Pg, P, B, w, prm = ref["Pg"], ref["P"], ref["B"], ref["work"], ref["prm"]
    own = owners(decomp_of(2), Pg)
    ids = Pg["ID"]
    row_of = {int(i): k for k, i in enumerate(ids)}
    holes = np.flatnonzero(Pg["Type"] == 5)
    hid = np.sort(ids[holes].astype(np.int64))
    c = dict(consecutive=int((np.diff(hid) == 1).sum()), swallower_left=0, swallower_right=0, grown_ghost=0, chain=0, heated_by_both=0, kicked_by_both=0,
             drawn_by_both_remote=0)
    for h in holes:                                          # swallowed holes whose swallower lives on the other rank
        mark = int(w["BH_SwallowID"][Pg["PI"][h]])
        if mark == 0 or (P["Flags"][h] & 2) == 0:
            continue
        s = row_of[mark - 1]
        if own[s] != own[h]:
            assert ids[s] > ids[h] or not is_timebin_active(Pg["TimeBinHydro"][h], TI)
            c["swallower_left" if own[s] == 0 else "swallower_right"] += 1
            growth = ref["acc_mass"][Pg["PI"][h]] / ref["Bg"]["Mass"][Pg["PI"][h]] - 1
            c["grown_ghost"] += int(h in ref["queue"] and growth > 1e-6)
    first = np.cumsum([0] + [r["nq"] for r in results])
    for rank, r in enumerate(results):
        m, e = r["marks"], r["effects"]
        msrc = np.searchsorted(first, m["hole"], side="right") - 1
        esrc = np.searchsorted(first, e["hole"], side="right") - 1
        for p in np.unique(m["part_index"][m["kind"] == 0]):           # a hole with candidates from both ranks: the chain's middle
            c["chain"] += len(np.unique(msrc[(m["part_index"] == p) & (m["kind"] == 0)])) > 1
        for p in np.unique(m["part_index"][m["kind"] == 1]):           # gas drawn by holes of both ranks, the winner not the gas's rank
            sel = (m["part_index"] == p) & (m["kind"] == 1)
            c["drawn_by_both_remote"] += len(np.unique(msrc[sel])) > 1 and msrc[sel][np.argmax(m["id"][sel])] != rank
        for kind, key in ((2, "heated_by_both"), (3, "kicked_by_both")):
            for p in np.unique(e["part_index"][e["kind"] == kind]):
                c[key] += len(np.unique(esrc[(e["part_index"] == p) & (e["kind"] == kind)])) > 1
    return c
