"""Brute-force numpy restatements of the three parts of the sharded metal return (shq_metal_return_triples / _apply / _sums) and the
set builder of its tests.  TEST INFRASTRUCTURE ONLY.

The arithmetic is oracle/metal_return.py's, expression by expression, so that the parts applied in global queue order give the bits
of its serial loop: `triples` meets the pairs of metal_return_ngbiter (r2 > 0, r2 < H^2, live gas) and routes them, `apply` runs the
body of the loop per gas particle with its stars in ascending global position, `sums` adds per star in (owner, particle) order."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from blackhole import kernel_wk, nearest  # noqa: E402

NMETALS = 9
NMESH = 48
MAXGASMASS = 4.0
SEED = 1


def triples(Pall, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, sphweighting, kt, box):
    """(owner, part_index, star, wk) of every (star of the queue, live gas particle inside its kernel) pair, sorted by the first three"""
    from shenqi_amd import capi
    live = ((Pall["Flags"] & 1) == 0) & (Pall["Type"] == 0)
    out = []
    for t, i in enumerate(queue):
        H = float(Pall["Hsml"][i])
        d = nearest(Pall["Pos"][i][None, :] - Pall["Pos"], box)
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        for other in np.flatnonzero(live & (r2 > 0) & (r2 < H * H)):
            wk = kernel_wk(np.sqrt(r2[other]) * (1.0 / H), H, kt) if sphweighting else 1.0
            own = other < nlocal
            out.append((rank if own else int(ghost_owner[other - nlocal]), int(other) if own else int(ghost_index[other - nlocal]), queue_offset + t, 0, wk))
    trip = np.array(out, dtype=capi.METAL_TRIPLE_DTYPE) if out else np.zeros(0, dtype=capi.METAL_TRIPLE_DTYPE)
    trip = trip[np.lexsort((trip["star"], trip["part_index"], trip["owner"]))]
    return trip, np.bincount(trip["owner"], minlength=nranks).astype(np.int64)


def apply(P, S, trip, table, maxgasmass):
    """the body of metal_return_ngbiter (oracle/metal_return.py:33-48) per triple, a particle's stars in ascending global position.
    Returns (thismass in the order of `trip`, refused flags, the smallest |mass + thismass - maxgasmass| met)."""
    thismass_out = np.zeros(len(trip))
    refused = np.zeros(len(trip), dtype=bool)
    margin = np.inf
    for k in np.lexsort((trip["star"], trip["part_index"])):
        other, t, wk = int(trip["part_index"][k]), int(trip["star"][k]), float(trip["wk"][k])
        starvolume, massgen, metalgen, speciesgen = table[t, 0], table[t, 1], table[t, 2], table[t, 3:]
        pi = int(P["PI"][other])
        mass = np.float32(P["Mass"][other])
        volume = float(mass) / S["Density"][pi]
        rf = wk * volume / starvolume
        thismass = rf * massgen
        margin = min(margin, abs(float(mass) + thismass - maxgasmass))
        if float(mass) + thismass > maxgasmass:
            refused[k] = True
            continue
        for m in range(NMETALS):
            tm = rf * speciesgen[m]
            S["Metals"][pi][m] = np.float32((float(np.float32(S["Metals"][pi][m]) * mass) + tm) / (float(mass) + thismass))
        thismetal = rf * metalgen
        S["Metallicity"][pi] = (S["Metallicity"][pi] * float(mass) + thismetal) / (float(mass) + thismass)
        massfrac = (float(mass) + thismass) / float(mass)
        P["Mass"][other] = np.float32(float(mass) * massfrac)
        S["Density"][pi] *= massfrac
        thismass_out[k] = thismass
    return thismass_out, refused, margin


def sums(qpos, owner, part_index, thismass, nqueue):
    out = np.zeros(nqueue)
    for k in np.lexsort((part_index, owner, qpos)):
        out[qpos[k]] += thismass[k]
    return out


class RestatedMetalOps:
    """DistMetalReturn's operators on the CPU; keeps what the tests assert about their own inputs"""

    def __init__(self, box):
        self.box = box
        self.received = self.refused = None
        self.margin = np.inf

    def stellar_density(self, Pall, Sall, queue, params):
        import orc
        import shenqi_amd as sq
        pman = sq.PartManager(len(Pall), self.box)
        pman.Base[:] = Pall
        tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
        st = orc.SphState(pman.Base, Sall)
        rc, vol, _, _ = orc.stellar_density(tree.Nodes_base, tree.firstnode, st, queue, self.box, params.DesNumNgb, params.MaxNgbDeviation, params.SPHWeighting,
                                            params.DensityKernelType)
        assert rc == 0
        Pall["Hsml"][queue] = st.hsml[queue]
        return vol[queue], None          # the oracle does not report the radii it tried

    def triples(self, Pall, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, sphweighting, kt):
        return triples(Pall, nlocal, queue, ghost_owner, ghost_index, nranks, rank, queue_offset, sphweighting, kt, self.box)

    def apply(self, P, S, trip, table, maxgasmass):
        tm, self.refused, self.margin = apply(P, S, trip, table, maxgasmass)
        self.received = trip.copy()
        return tm

    def sums(self, qpos, owner, part_index, thismass, nqueue):
        return sums(qpos, owner, part_index, thismass, nqueue)


def global_set(seed=SEED, sphw=0, kt=1, hscale=2.4, **kw):
    """test_gpu_metal_return.setup's set: (P, S, queue, per-star rows [nq, 12]) - gas on a jittered lattice, dying stars, some crowded.
    hscale = 2.4 gives every gas particle several returns, so that the heavy ones (Mass 3.9) run into MaxGasMass = 4 and some returns
    are refused; setup's StarVolumeSPH is a plain volume sum, so with the kernel weight it is scaled by the weight at half the star's
    kernel radius: the returns, and the refusals, then stay of the same size."""
    import test_gpu_metal_return as tmr
    pman, S, queue, starvol, massgen, metalgen, species = tmr.setup(seed, hscale=hscale, **kw)
    if sphw:
        starvol = starvol * np.array([kernel_wk(0.5, float(h), kt) for h in pman.Base["Hsml"][queue]])
    return pman.Base.copy(), S, queue, np.concatenate([starvol[:, None], massgen[:, None], metalgen[:, None], species], axis=1)


def owners(decomp, P):
    return decomp.owner_of(torch.from_numpy(np.ascontiguousarray(P["Pos"][:, 0]))).numpy()


def local_part(rank, decomp, Pg, Sg, queueg, rowsg, keep_queue=True):
    """this rank's share of the global set: its particles, their slots renumbered locally, the stars of the global queue it owns
    (in the global queue's order) with their rows.  Also returns the global rows of its particles and of its queue."""
    mine = np.flatnonzero(owners(decomp, Pg) == rank)
    P = Pg[mine].copy()
    gas, star = P["Type"] == 0, P["Type"] == 4
    S = Sg[P["PI"][gas]].copy()
    P["PI"][gas] = np.arange(gas.sum())
    P["PI"][star] = np.arange(star.sum())
    back = {int(g): k for k, g in enumerate(mine)}
    sel = [k for k, g in enumerate(queueg) if int(g) in back] if keep_queue else []
    queue = np.array([back[int(queueg[k])] for k in sel], dtype=np.int32)
    return P, S, queue, rowsg[sel].copy(), mine, np.asarray(queueg)[sel]


def global_order(decomp, Pg, queueg, nranks, empty=()):
    """positions in queueg of the global queue the sharded run applies: the ranks' queues one after the other, in rank order"""
    own = owners(decomp, Pg)[queueg]
    return np.concatenate([np.flatnonzero(own == r) if r not in empty else np.zeros(0, dtype=np.int64) for r in range(nranks)]).astype(np.int64)


def run_rank(comm, rank, ops, sphw, kt=1, seed=SEED, empty=(), **kw):
    """one rank of DistMetalReturn.run on global_set(seed); ranks in `empty` run with an empty queue"""
    import common as cm
    from shenqi_amd import dist as sd
    Pg, Sg, queueg, rowsg = global_set(seed, sphw, kt, **kw)
    decomp = sd.SlabDecomp(comm, NMESH, cm.BOX)
    P, S, queue, rows, mine, _ = local_part(rank, decomp, Pg, Sg, queueg, rowsg, keep_queue=rank not in empty)
    drv = sd.DistMetalReturn(comm, decomp, ops)
    mret = drv.run(P, S, queue, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:], MAXGASMASS, sphw, kt)
    gas = P["Type"] == 0
    pi = P["PI"][gas]
    return dict(rows=mine, mass=P["Mass"].copy(), gas_rows=mine[gas], density=S["Density"][pi], metallicity=S["Metallicity"][pi], metals=S["Metals"][pi],
                mret=mret, nq=len(queue), nghost=drv.nghost, ntriples_sent=drv.ntriples_sent,
                received=getattr(ops, "received", None), refused=getattr(ops, "refused", None), margin=getattr(ops, "margin", None))


def compare(results, ref, Pg, queueg, order, exact_gas=True):
    """results of all ranks against ref = (P, S, MassReturn) of the undivided run with the queue queueg[order]; returns the largest
    differences (mass, density, metallicity, metals relative to the largest value; MassReturn relative to its largest)"""
    P, S, mret = ref
    worst = dict(mass=0.0, density=0.0, metallicity=0.0, metals=0.0, mret=0.0)
    seen, got = 0, []
    for r in results:
        seen += len(r["rows"])
        pi = Pg["PI"][r["gas_rows"]]
        for key, a, b in (("mass", r["mass"], P["Mass"][r["rows"]]), ("density", r["density"], S["Density"][pi]),
                          ("metallicity", r["metallicity"], S["Metallicity"][pi]), ("metals", r["metals"], S["Metals"][pi])):
            if exact_gas:
                assert np.array_equal(a, b), key
            worst[key] = max(worst[key], float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max()))
        got.append(r["mret"])
    assert seen == len(P)
    got = np.concatenate(got)
    assert len(got) == len(order)
    worst["mret"] = float(np.abs(got - mret).max() / mret.max())
    assert worst["mret"] <= 1e-14
    return worst


def stars_set(third=False):
    """test_oracle_cpu._stars_in_gas with the stars' Hsml converged by the undivided oracle (third: a third of that, so that the first
    halo is too small): (P, SphP, first star row, number of stars, params)"""
    from types import SimpleNamespace
    import common as cm
    import orc
    import shenqi_amd as sq
    import test_oracle_cpu as toc
    pman, SphP, ng, nstar = toc._stars_in_gas(n1=14, nstar=200, seed=7)
    prm = SimpleNamespace(DesNumNgb=4.0 / 3 * np.pi * 2.0**3, MaxNgbDeviation=2.0, SPHWeighting=1, DensityKernelType=1)
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    queue = np.arange(ng, ng + nstar, dtype=np.int32)
    st = orc.SphState(pman.Base, SphP)
    rc = orc.stellar_density(tree.Nodes_base, tree.firstnode, st, queue, cm.BOX, prm.DesNumNgb, prm.MaxNgbDeviation, prm.SPHWeighting, prm.DensityKernelType)[0]
    assert rc == 0
    P = pman.Base.copy()
    P["Hsml"][queue] = st.hsml[queue] / (3.0 if third else 1.0)
    return P, SphP, ng, nstar, prm


def stars_reference(P, SphP, ng, nstar, prm):
    """the undivided oracle from the set's Hsml: (final Hsml, StarVolumeSPH) of the stars"""
    import common as cm
    import orc
    import shenqi_amd as sq
    pman = sq.PartManager(len(P), cm.BOX)
    pman.Base[:] = P
    tree = sq.force_tree_rebuild_mask(pman, sq.GASMASK)
    queue = np.arange(ng, ng + nstar, dtype=np.int32)
    st = orc.SphState(pman.Base, SphP)
    rc, vol, _, _ = orc.stellar_density(tree.Nodes_base, tree.firstnode, st, queue, cm.BOX, prm.DesNumNgb, prm.MaxNgbDeviation, prm.SPHWeighting, prm.DensityKernelType)
    assert rc == 0
    return st.hsml[queue].copy(), vol[queue].copy()


def run_rank_stars(comm, rank, ops, third):
    import common as cm
    from shenqi_amd import dist as sd
    Pg, Sg, ng, nstar, prm = stars_set(third)
    decomp = sd.SlabDecomp(comm, NMESH, cm.BOX)
    queueg = np.arange(ng, ng + nstar, dtype=np.int32)
    P, S, queue, _, mine, qrows = local_part(rank, decomp, Pg, Sg, queueg, np.zeros((nstar, 1)))
    drv = sd.DistMetalReturn(comm, decomp, ops)
    vol, rounds = drv.stellar_density(P, S, queue, prm)
    return dict(stars=qrows - ng, hsml=P["Hsml"][queue].copy(), vol=vol, rounds=rounds, nghost=drv.nghost)


def compare_stars(results, third, ref=None):
    """Hsml and StarVolumeSPH of all ranks' stars against the undivided result (ref = (Hsml, StarVolumeSPH) by star; default: the oracle's)"""
    Pg, Sg, ng, nstar, prm = stars_set(third)
    hs, vol = ref if ref is not None else stars_reference(Pg, Sg, ng, nstar, prm)
    seen = 0
    worst = [0.0, 0.0]
    for r in results:
        seen += len(r["stars"])
        worst[0] = max(worst[0], float(np.abs(r["hsml"] / hs[r["stars"]] - 1).max()))
        worst[1] = max(worst[1], float(np.abs(r["vol"] / vol[r["stars"]] - 1).max()))
    assert seen == nstar
    assert worst[0] < 1e-9 and worst[1] < 1e-9, worst
    return worst
