"""turn_on_quasars (libgadget/cooling_qso_lightup.cpp:489-596) as its loop runs on several tasks, restated in numpy on the undivided
particle set: the yardstick of shenqi_amd/dist.py:DistHeIII.  heiii_restated.py (one task) supplies the particle test, the heating and
the libm calls.

On R tasks every task holds its own candidate list (the groups it hosts, in the order given), its own ncand_before and the global
ncand_tot; all draw the same global position.  choose_QSO_halo decrements ncand_before before its range test, so the task behind the
drawn one can return local index 0 for a position it does not host, erase its candidate 0 without walking, and leave positions nobody
hosts behind.  turn_on_quasars_ranks keeps R independent replays of those counters and works one iteration and one bubble at a time.
The walk of the hosting task reaches the gas of every task, so a bubble is one mask over all gas, whoever holds it.

Also here: RestatedHeiiiOps (DistHeIII's four operations in numpy, so that the driver runs without a device), the test set
(global_set) and run_rank, shared by tests/test_dist_heiii_cpu.py and tests/test_gpu_dist_heiii.py."""
import math

import numpy as np

from shenqi_amd import capi
from shenqi_amd import dist as sd
import heiii_restated as hr

BOX = 20000.0
FIRST_BATCH, MAX_BATCH = 32, 1024


def _wrapped(cm, offset, box):
    qp = []
    for d in range(3):
        x = cm[d] - offset[d]
        if math.isfinite(x):
            while x > box:
                x -= box
            while x <= 0:
                x += box
        qp.append(x)
    return tuple(qp)


def turn_on_quasars_ranks(pos, types, flags, pi, density, entropy, rank_groups, TotNgroups, rnd, P, part_rank=None):
    """rank_groups: per task the catalogue it hosts (FOF_GROUP_DTYPE: Mass, MinID, CM) in the order given; TotNgroups: the global group
    count; P: dict of shq_heiii_params' fields, n_gas_tot global.  part_rank: the task holding each particle (for the event counts only).
    Returns (flags, entropy, log, result, events): log lines are (host task, local group index, pos[3], ionfrac, n_ionized), with
    (-1, -1, zeros) when no task walked.  events: iterations in which two tasks had new_qso >= 0 (two_host), no task had (unhosted),
    some task had 0 and none walked (index0); after_two_host_unhosted: unhosted draws after the first two-host iteration; bubbles whose
    ionised particles lie on more than one task (split_bubbles), and of those the ones that ionised through the periodic x face
    (face_split); idle: (batch, task) pairs of the 32, 64, ... schedule, batch fully run, where the task still had eligible gas and no
    lit bubble of the batch held any gas particle of that task."""
    flags = np.array(flags, dtype=np.uint8, copy=True)
    entropy = np.array(entropy, dtype=np.float64, copy=True)
    R_ = len(rank_groups)
    box = P["BoxSize"]
    n_gas_tot = int(P["n_gas_tot"])
    a3inv = 1 / hr._libm.pow(P["atime"], 3)
    nheperg = (1 - hr.HYDROGEN_MASSFRAC) / (hr.PROTONMASS * hr.HEMASS)
    deltau = P["qso_inst_heating"] * nheperg
    uu = P["uu_in_cgs"]
    desired = P["desired_ion_frac"]
    gas = types == 0
    if part_rank is None:
        part_rank = np.zeros(len(pos), dtype=np.int64)
    res = dict(init_ionfrac=0.0, final_ionfrac=0.0, n_candidates=0, n_iterations=0, n_flash=0, n_ionized=0)
    ev = dict(two_host=0, unhosted=0, index0=0, after_two_host_unhosted=0, split_bubbles=0, face_split=0, idle=0)
    if desired > P["heIIIreion_finish_frac"]:    # the flash is local to every task: together, every Type-0 particle
        idx = np.flatnonzero(gas & ((flags & hr.FLAG_HEIII) == 0))
        hr._heat(idx, flags, entropy, pi, density, a3inv, deltau, uu)
        res["n_flash"] = len(idx)
    rhobar = P["OmegaBaryon"] * (3 * hr.HUBBLE * P["HubbleParam"] * hr.HUBBLE * P["HubbleParam"]) / (8 * math.pi * hr.GRAVITY) * a3inv
    totbubblegasmass = 4 * math.pi / 3. * hr._libm.pow(P["mean_bubble"], 3) * rhobar
    non_overlapping_bubble_number = int(n_gas_tot * totbubblegasmass / P["OmegaBaryon"])
    cur = int(np.count_nonzero(gas & ((flags & hr.FLAG_HEIII) != 0))) / n_gas_tot
    res["init_ionfrac"] = res["final_ionfrac"] = cur
    log = []
    qso_cand = [[] for _ in range(R_)]
    if cur < desired:
        for r, groups in enumerate(rank_groups):
            qso_cand[r] = [g for g in range(len(groups))
                           if not (groups["Mass"][g] < P["qso_candidate_min_mass"]) and not (groups["Mass"][g] > P["qso_candidate_max_mass"])]
    ncand = [len(c) for c in qso_cand]
    ncand_tot = sum(ncand)
    ncand_before = [sum(ncand[:r]) for r in range(R_)]     # count_QSO_halos
    res["n_candidates"] = ncand_tot
    if ncand_tot == 0:
        return flags, entropy, log, res, ev
    sigma = hr._libm.sqrt(P["var_bubble"])
    tot = 0
    iteration = 0
    batch_end, batch_len = FIRST_BATCH, FIRST_BATCH
    touched = np.zeros(R_, dtype=bool)     # tasks some lit bubble of the running batch held a gas particle of
    lit_in_batch = 0
    while cur < desired:
        drand = rnd[(TotNgroups + iteration) % len(rnd)]
        qso = int(drand * ncand_tot)
        ncand_tot -= 1
        new_qso = []
        for r in range(R_):               # every task's own choose_QSO_halo
            if qso < ncand_before[r]:
                ncand_before[r] -= 1
            new_qso.append(-1 if (qso < ncand_before[r] or qso >= ncand_before[r] + len(qso_cand[r])) else qso - ncand_before[r])
        if ncand_tot <= 0:
            break
        hosts = [r for r in range(R_) if new_qso[r] >= 0]
        walkers = [r for r in range(R_) if new_qso[r] > 0]
        assert len(walkers) <= 1
        ev["two_host"] += len(hosts) >= 2
        ev["unhosted"] += len(hosts) == 0
        ev["after_two_host_unhosted"] += len(hosts) == 0 and ev["two_host"] > 0
        ev["index0"] += len(hosts) > 0 and not walkers
        n_ionized = 0
        line = (-1, -1, (0.0, 0.0, 0.0))
        if walkers:
            r = walkers[0]
            group = qso_cand[r][new_qso[r]]
            groups = rank_groups[r]
            cm = [float(x) for x in groups["CM"][group]]
            Rb = hr.gaussian_rng(P["mean_bubble"], sigma, int(groups["MinID"][group]), rnd)
            if Rb < 0:
                raise ValueError("a negative radius: membership would depend on each task's tree")
            with np.errstate(invalid="ignore", over="ignore"):
                tx = cm[0] - pos[:, 0]
                dx = hr.nearest(tx, box)
                dy = hr.nearest(cm[1] - pos[:, 1], box)
                dz = hr.nearest(cm[2] - pos[:, 2], box)
                r2 = dx * dx
                r2 = r2 + dy * dy
                r2 = r2 + dz * dz
                inside = ~(r2 > Rb * Rb)
            idx = np.flatnonzero(gas & ((flags & (hr.FLAG_GARBAGE | hr.FLAG_HEIII)) == 0) & inside)
            hr._heat(idx, flags, entropy, pi, density, a3inv, deltau, uu)
            n_ionized = len(idx)
            on = np.unique(part_rank[idx])
            ev["split_bubbles"] += len(on) > 1
            ev["face_split"] += len(on) > 1 and bool(np.any(dx[idx] != tx[idx]))
            touched[np.unique(part_rank[np.flatnonzero(gas & inside)])] = True
            lit_in_batch += 1
            line = (r, group, _wrapped(cm, P["CurrentParticleOffset"], box))
        cur += n_ionized / n_gas_tot
        tot += n_ionized
        log.append(line + (cur, n_ionized))
        if n_ionized < 0.01 * non_overlapping_bubble_number and iteration > 10:
            break
        for r in hosts:
            del qso_cand[r][new_qso[r]]
        iteration += 1
        if iteration == batch_end:        # a batch of the 32, 64, ... schedule ran to its end
            if lit_in_batch:
                elig = gas & ((flags & (hr.FLAG_GARBAGE | hr.FLAG_HEIII)) == 0)
                ev["idle"] += sum(1 for r in range(R_) if not touched[r] and np.any(elig & (part_rank == r)))
            batch_len = min(2 * batch_len, MAX_BATCH)
            batch_end += batch_len
            touched[:] = False
            lit_in_batch = 0
    res.update(final_ionfrac=cur, n_iterations=len(log), n_ionized=tot)
    return flags, entropy, log, res, ev


class RestatedHeiiiOps:
    """DistHeIII's open / sweep / commit / close in numpy, with heiii_restated's particle test and heating"""

    def __init__(self, cull=True):
        self.cull = cull

    def open(self, P, SphP, p):
        self.flags, self.entropy = P["Flags"].copy(), SphP["Entropy"].copy()
        self.pos, self.pi, self.density, self.box = P["Pos"], P["PI"], SphP["Density"], p.BoxSize
        self.a3inv = 1 / hr._libm.pow(p.atime, 3)
        self.deltau = p.qso_inst_heating * ((1 - hr.HYDROGEN_MASSFRAC) / (hr.PROTONMASS * hr.HEMASS))
        self.uu = p.uu_in_cgs
        gas = P["Type"] == 0
        n_flash = 0
        if p.desired_ion_frac > p.heIIIreion_finish_frac:
            idx = np.flatnonzero(gas & ((self.flags & hr.FLAG_HEIII) == 0))
            self._heat(idx)
            n_flash = len(idx)
        self.nrows = n_flash
        nion = int(np.count_nonzero(gas & ((self.flags & hr.FLAG_HEIII) != 0)))
        self.elig = np.flatnonzero(gas & ((self.flags & (hr.FLAG_GARBAGE | hr.FLAG_HEIII)) == 0))
        self.hit = None
        x = self.pos[self.elig]
        lo = x.min(axis=0) if len(x) else np.full(3, np.inf)
        hi = x.max(axis=0) if len(x) else np.full(3, -np.inf)
        return n_flash, nion, len(self.elig), lo, hi

    def _heat(self, idx):
        hr._heat(idx, self.flags, self.entropy, self.pi, self.density, self.a3inv, self.deltau, self.uu)

    def sweep(self, bubbles, nseq):
        x = self.pos[self.elig]
        self.hit = np.full(len(x), -1, dtype=np.int64)
        for b in bubbles:
            assert not b["R"] < 0
            with np.errstate(invalid="ignore", over="ignore"):
                dx = hr.nearest(float(b["c"][0]) - x[:, 0], self.box)
                dy = hr.nearest(float(b["c"][1]) - x[:, 1], self.box)
                dz = hr.nearest(float(b["c"][2]) - x[:, 2], self.box)
                r2 = dx * dx
                r2 = r2 + dy * dy
                r2 = r2 + dz * dz
                inside = ~(r2 > float(b["R"]) * float(b["R"]))
            self.hit[(self.hit < 0) & inside] = int(b["seq"])
        return np.bincount(self.hit[self.hit >= 0], minlength=nseq).astype(np.uint64)

    def commit(self, seq_stop):
        sel = (self.hit >= 0) & (self.hit < seq_stop)
        self._heat(self.elig[sel])
        self.elig, self.hit = self.elig[~sel], None
        self.nrows += int(sel.sum())
        return int(sel.sum())

    def close(self, P, SphP):
        P["Flags"], SphP["Entropy"] = self.flags, self.entropy
        return self.nrows


# ---- the test set ----
CUTS = {1: (0.0, 1.0), 2: (0.0, 0.62, 1.0), 3: (0.0, 0.3, 0.62, 1.0)}       # x-slabs of the tasks, in units of the box
# seed and rnd_seed: the first pair of a search over the restatement alone for which the two- and the three-task run both hold every
# event tests/test_dist_heiii_cpu.py asserts (about one pair in a hundred does)
DEFAULT = dict(N=14, seed=3, rnd_seed=8, world=2, mean_bubble=1500.0, var_bubble=0.0, stop_iter=45, desired_ion_frac=None, flash=False,
               no_groups=(), no_gas=(), min_mass=5.0, u1_zero=0)
_sets = {}


def params_dict(ngas, **kw):
    p = dict(BoxSize=BOX, atime=0.25, qso_candidate_min_mass=5.0, qso_candidate_max_mass=1e30, mean_bubble=1500.0, var_bubble=0.0,
             heIIIreion_finish_frac=0.995, desired_ion_frac=0.9, qso_inst_heating=2e-12, uu_in_cgs=1e10, OmegaBaryon=0.045,
             HubbleParam=0.7, CurrentParticleOffset=(1234.5, -777.25, 20001.0), n_gas_tot=ngas)
    p.update(kw)
    return p


def params_struct(p):
    s = capi.HeiiiParams()
    for k, v in p.items():
        if k == "CurrentParticleOffset":
            for d in range(3):
                s.CurrentParticleOffset[d] = v[d]
        else:
            setattr(s, k, v)
    return s


def global_set(**case):
    """The undivided set of a case (cached, never modified): 2 N^3 particles, half of them gas, no two sharing a coordinate (every axis
    is a permutation of 2 N^3 distinct levels); some gas garbage, some ionised already, Generation and BHHeated bits set here and
    there.  60 candidate groups and 10 below the mass window; most candidates sit at x in [0.10, 0.52] of the box, two next to the
    periodic x face and two inside the last slab, so that the last task is out of reach of most bubbles.  The groups are dealt to
    the tasks in a shuffled order, whatever their position."""
    c = dict(DEFAULT, **case)
    key = repr(sorted(c.items()))
    if key in _sets:
        return _sets[key]
    rng = np.random.default_rng(c["seed"])
    W, n = c["world"], 2 * c["N"] ** 3
    pos = np.stack([(rng.permutation(n) + 0.5) * (BOX / n) for _ in range(3)], axis=1)
    types = np.ones(n, dtype=np.uint8)
    types[rng.choice(n, n // 2, replace=False)] = 0
    part_rank = np.searchsorted(np.array(CUTS[W][1:-1]) * BOX, pos[:, 0], side="right")
    for r in c["no_gas"]:
        types[part_rank == r] = 1
    gas_idx = np.flatnonzero(types == 0)
    Pg = np.zeros(n, dtype=capi.PARTICLE_DTYPE)
    Pg["Pos"], Pg["Type"], Pg["Mass"] = pos, types, np.where(types == 0, 0.2, 1.0)
    Pg["ID"] = rng.permutation(n).astype(np.uint64) + 1
    Pg["Hsml"] = BOX / c["N"]
    Pg["PI"][gas_idx] = np.arange(len(gas_idx))
    flags = (rng.integers(0, 16, n) << 4).astype(np.uint8)
    flags |= np.where(rng.random(n) < 0.1, 8, 0).astype(np.uint8)
    flags[rng.choice(gas_idx, max(n // 200, 2), replace=False)] |= 1
    flags[rng.choice(gas_idx, max(n // 100, 2), replace=False)] |= 4
    Pg["Flags"] = flags
    Sg = np.zeros(len(gas_idx), dtype=capi.SPH_DTYPE)
    Sg["Density"] = rng.uniform(0.5, 50.0, len(Sg))
    Sg["Entropy"] = rng.uniform(1.0, 10.0, len(Sg))
    ncand, nlow = 60, 10
    G = np.zeros(ncand + nlow, dtype=capi.FOF_GROUP_DTYPE)
    G["MinID"] = rng.permutation(1 << 20)[:len(G)].astype(np.uint64) + 7
    G["Mass"][:ncand] = rng.uniform(10.0, 100.0, ncand)
    G["Mass"][ncand:] = rng.uniform(0.5, 4.0, nlow)
    cx = rng.uniform(0.10, 0.52, len(G))
    cx[:2] = rng.uniform(0.004, 0.03, 2)
    cx[2:4] = rng.uniform(0.72, 0.9, 2)
    G["CM"] = np.stack([cx, rng.uniform(0, 1, len(G)), rng.uniform(0, 1, len(G))], axis=1) * BOX
    G = G[rng.permutation(len(G))]
    share = np.array([0.0, 1.0]) if W == 1 else (np.array([0.0, 0.55, 1.0]) if W == 2 else np.array([0.0, 0.38, 0.68, 1.0]))
    bounds = np.round(share * len(G)).astype(int)
    rank_groups = [G[bounds[r]:bounds[r + 1]].copy() for r in range(W)]
    for r in c["no_groups"]:
        rank_groups[r] = G[:0].copy()
    rnd = np.random.default_rng(c["rnd_seed"]).random(4096)
    for k in range(c["u1_zero"]):         # gaussian_rng's u1 = 0 for the first candidates of task 0, with cos(2 pi u2) > 0: +inf under var > 0
        mid = int(rank_groups[0]["MinID"][np.flatnonzero(rank_groups[0]["Mass"] >= 5.0)[1 + k]])
        rnd[mid % len(rnd)], rnd[(mid + 1) % len(rnd)] = 0.0, 0.05
    ngas = len(Sg)
    p = params_dict(ngas, mean_bubble=c["mean_bubble"], var_bubble=c["var_bubble"], qso_candidate_min_mass=c["min_mass"])
    if c["flash"]:
        p["desired_ion_frac"] = 0.999
    elif c["desired_ion_frac"] is not None:
        p["desired_ion_frac"] = c["desired_ion_frac"]
    else:    # a target the loop reaches at iteration stop_iter, or at the first one after it that ionises
        probe = turn_on_quasars_ranks(pos, types, flags, Pg["PI"], Sg["Density"], Sg["Entropy"], rank_groups, len(G), rnd, dict(p, desired_ion_frac=0.99))
        k = next(i for i in range(c["stop_iter"], len(probe[2])) if probe[2][i][4] > 0)
        p["desired_ion_frac"] = probe[2][k][3]
    out = dict(Pg=Pg, Sg=Sg, part_rank=part_rank, rank_groups=rank_groups, TotNgroups=len(G), params=p, rnd=rnd, world=W)
    _sets[key] = out
    return out


_refs = {}


def reference(**case):
    """turn_on_quasars_ranks on the undivided set of the case, computed once and left unchanged"""
    key = repr(sorted(dict(DEFAULT, **case).items()))
    if key not in _refs:
        s = global_set(**case)
        Pg, Sg = s["Pg"], s["Sg"]
        _refs[key] = turn_on_quasars_ranks(Pg["Pos"], Pg["Type"], Pg["Flags"], Pg["PI"], Sg["Density"], Sg["Entropy"], s["rank_groups"], s["TotNgroups"],
                                           s["rnd"], s["params"], s["part_rank"])
    return _refs[key]


def run_rank(comm, rank, ops, case):
    """DistHeIII on this task's share of the case's set: its particles (in the set's order, PI renumbered to its own slots) and the
    groups it hosts.  Returns what the tests compare, and an exception's text instead of log and result when the driver raised."""
    s = global_set(**case)
    mine = np.flatnonzero(s["part_rank"] == rank)
    P = s["Pg"][mine].copy()
    gas = P["Type"] == 0
    slots = P["PI"][gas].copy()
    S = s["Sg"][slots].copy()
    P["PI"][gas] = np.arange(len(S))
    drv = sd.DistHeIII(comm, ops)
    out = dict(mine=mine, slots=slots, error=None, log=None, res=None)
    try:
        out["log"], out["res"] = drv.run(P, S, s["rank_groups"][rank], s["TotNgroups"], params_struct(s["params"]), s["rnd"])
    except ValueError as e:
        out["error"] = str(e)
    out.update(flags=P["Flags"].copy(), entropy=S["Entropy"].copy(), nsweeps=drv.nsweeps, kept=list(drv.kept), ntests=drv.ntests, nrows=drv.nrows,
               events=dict(drv.events))
    return out


def assemble(results, case):
    """the tasks' flags and entropies in the undivided set's order"""
    s = global_set(**case)
    flags, entropy = s["Pg"]["Flags"].copy(), s["Sg"]["Entropy"].copy()
    for r in results:
        flags[r["mine"]] = r["flags"]
        entropy[r["slots"]] = r["entropy"]
    return flags, entropy
