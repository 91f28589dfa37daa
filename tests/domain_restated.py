"""The reference's domain decomposition (libgadget/domain.cpp) restated in plain Python, serial loops as the reference writes them:
what the device operators of shenqi_amd/csrc/domain.hip, the host stages of domain_host.hpp and the DistDomain driver are held to.

Unpinned: the reference holds no domain test, and domain.cpp does not build here without stand-ins for MPI, so nothing in this file
is compared with a reference binary.  What is pinned is the key: peano_key() walks the automaton tables that
shq_peano_tables_from_key recovers from the reference's own peano_hilbert_key (oracle/_ref/libpeano_ref.so where built, the tables of
tests/golden/ref_domain.npz otherwise, which must reproduce the hilbert_key tables of tests/golden/ref_peano.npz).

Line numbers are domain.cpp's unless another file is named."""
import os

import numpy as np

import ref_outputs as ro
from shenqi_amd import capi

BITS = 21
PEANOCELLS = 1 << 63
ROOT_SHIFT = 3 * BITS
DOMAIN_GOLD = os.path.join(ro.GOLD, "ref_domain.npz")
NPOLICY = 16


# ---- the key -------------------------------------------------------------------------------------------------------------------
def reference_keyfn():
    """ctypes pointer to the reference's peano_hilbert_key (oracle/ref_peano_driver.cpp), or None where oracle/_ref is not built"""
    lib = ro.peano_lib()
    return None if lib is None else lib.ref_peano_hilbert_key


def tables():
    """(PeanoTables, next, sub): derived from the reference's function where it is built, the stored derivation otherwise"""
    fn = reference_keyfn()
    if fn is not None:
        t = capi.peano_tables_from_key(fn)
    else:
        g = np.load(DOMAIN_GOLD)
        t = capi.peano_tables_from_arrays(g["next"], g["sub"])
    nxt, sub = capi.peano_tables_to_arrays(t)
    return t, nxt, sub


def peano_key(nxt, sub, x, y, z, bits=BITS):
    """peano_hilbert_key(x, y, z, bits) through the automaton, vectorised over integer arrays"""
    x, y, z = (np.asarray(a, dtype=np.int64) for a in (x, y, z))
    key = np.zeros(x.shape, dtype=np.uint64)
    s = np.zeros(x.shape, dtype=np.int64)
    for b in range(bits - 1, -1, -1):
        o = (((x >> b) & 1) << 2) | (((y >> b) & 1) << 1) | ((z >> b) & 1)
        key = (key << np.uint64(3)) | sub[s, o].astype(np.uint64)
        s = nxt[s, o].astype(np.int64)
    return key


def grid_coords(pos, box):
    """the integer coordinates PEANO() hands to peano_hilbert_key (utils/peano.h:15-21): the same three double operations, truncated"""
    pos = np.asarray(pos, dtype=np.float64)
    fac = np.float64(1.0) / (np.float64(box) * np.float64(1.001)) * np.float64(1 << BITS)
    return ((pos + np.float64(box) / np.float64(2000)) * fac).astype(np.int64)


def PEANO(nxt, sub, pos, box):
    g = grid_coords(pos, box)
    return peano_key(nxt, sub, g[:, 0], g[:, 1], g[:, 2])


# ---- subsample (:1005-1067) -----------------------------------------------------------------------------------------------------
def samples(keys, garbage, dist, presort):
    """keys: PEANO of every slot, garbage: bool per slot.  Returns the rank's samples, sorted locally (the reference sorts them across
    the ranks next; a local sort first changes nothing of that)."""
    n = len(keys)
    keys = np.asarray(keys, dtype=np.uint64)
    garbage = np.asarray(garbage, dtype=bool)
    if presort:
        full = np.where(garbage, np.uint64(PEANOCELLS), keys)
        full = np.sort(full, kind="stable")
        live = n - int(garbage.sum())
        ns = live // dist
        if ns == 0 and live > 0:
            ns = 1
        return full[np.arange(ns) * dist].copy()
    ns = n // dist
    if ns == 0 and n != 0:
        ns = 1
    j = np.arange(ns) * dist
    lp = keys[j][~garbage[j]]
    return np.sort(lp, kind="stable")


# ---- the local top tree (:819-958, :1073-1168) ---------------------------------------------------------------------------------
def new_node(StartKey=0, Shift=ROOT_SHIFT, Daughter=-1, Parent=-1, Count=0, Cost=0):
    return dict(StartKey=int(StartKey), Shift=int(Shift), Daughter=int(Daughter), Parent=int(Parent), Count=int(Count), Cost=int(Cost))


def get_subnode(T, key):
    no = 0
    while T[no]["Daughter"] >= 0:
        no = T[no]["Daughter"] + ((key - T[no]["StartKey"]) >> (T[no]["Shift"] - 3))
    return no


def insert(T, key, cost):
    leaf = get_subnode(T, key)
    T[leaf]["Count"] += 1
    T[leaf]["Cost"] += cost
    return leaf


def split(T, MaxTopNodes, i):
    if len(T) + 8 > MaxTopNodes:
        return 1
    assert T[i]["Shift"] >= 3
    T[i]["Daughter"] = len(T)
    sh = T[i]["Shift"] - 3
    for j in range(8):
        T.append(new_node(T[i]["StartKey"] + j * (1 << sh), sh, -1, i, 0, 0))
    return 0


def skeleton(lp, MaxTopNodes):
    """the serial loop of :1110-1149, then steps 2 and 3 and the sums up the tree; None when it runs out of top nodes"""
    T = [new_node()]
    last_key, last_leaf, i = None, -1, 0
    n = len(lp)
    while i < n:
        key = int(lp[i])
        leaf = get_subnode(T, key)
        if leaf == last_leaf and T[leaf]["Shift"] >= 3:
            if split(T, MaxTopNodes, leaf):
                return None
            T[leaf]["Count"] = 0
            last_leaf = insert(T, last_key, 0)
            continue
        assert not (T[leaf]["Count"] != 0 and leaf != last_leaf), "samples not sorted"
        last_key = key
        last_leaf = insert(T, last_key, 0)
        i += 1
    for nd in T:
        nd["Count"] = 0
    for k in lp:
        insert(T, int(k), 1)

    def update_cost(start):
        if T[start]["Daughter"] == -1:
            return
        for j in range(8):
            s = T[start]["Daughter"] + j
            update_cost(s)
            T[start]["Count"] += T[s]["Count"]
            T[start]["Cost"] += T[s]["Cost"]
    update_cost(0)
    return T


def truncate(T, countlimit, costlimit):
    """domain_toptree_truncate: truncate_r, then the garbage collection that moves the survivors to the front"""
    def trunc(start):
        if T[start]["Daughter"] == -1:
            return
        if T[start]["Count"] < countlimit and T[start]["Cost"] < costlimit:
            T[start]["Daughter"] = -1
            return
        for j in range(8):
            trunc(T[start]["Daughter"] + j)
    trunc(0)
    T = [dict(nd) for nd in T]
    size = [1]

    def gc(start):
        if T[start]["Daughter"] == -1:
            return
        oldd, newd = T[start]["Daughter"], size[0]
        T[start]["Daughter"] = newd
        size[0] += 8
        for j in range(8):
            T[newd + j] = dict(T[oldd + j])
            T[newd + j]["Parent"] = start
        for j in range(8):
            gc(newd + j)
    gc(0)
    return T[:size[0]]


def local_toptree(lp, countlimit, costlimit, MaxTopNodes):
    T = skeleton(lp, MaxTopNodes)
    return None if T is None else truncate(T, countlimit, costlimit)


def to_array(T):
    a = np.zeros(len(T), dtype=capi.LOCAL_TOPNODE_DTYPE)
    for f in ("StartKey", "Shift", "Daughter", "Parent", "Count", "Cost"):
        a[f] = [nd[f] for nd in T]
    return a


def from_array(a):
    return [new_node(*(int(r[f]) for f in ("StartKey", "Shift", "Daughter", "Parent", "Count", "Cost"))) for r in a]


def cdiv(a, b):
    """C's integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


# ---- domain_toptree_merge (:1447-1552) ------------------------------------------------------------------------------------------
class OutOfNodes(Exception):
    pass


def merge(A, B, MaxTopNodes, noA=0, noB=0):
    """treeB into treeA (lists of node dicts; A grows).  OutOfNodes where the reference ends the run for lack of room."""
    if B[noB]["Shift"] < A[noA]["Shift"]:
        if A[noA]["Daughter"] < 0:
            if len(A) + 8 > MaxTopNodes:
                raise OutOfNodes()
            pb = B[noB]["Parent"]
            count = A[noA]["Count"] - B[pb]["Count"]
            cost = A[noA]["Cost"] - B[pb]["Cost"]
            A[noA]["Daughter"] = len(A)
            sh = A[noA]["Shift"] - 3
            for j in range(8):
                A.append(new_node(A[noA]["StartKey"] + j * (1 << sh), sh, -1, noA, cdiv((j + 1) * count, 8) - cdiv(j * count, 8),
                                  cdiv((j + 1) * cost, 8) - cdiv(j * cost, 8)))
        sub = A[noA]["Daughter"] + ((B[noB]["StartKey"] - A[noA]["StartKey"]) >> (A[noA]["Shift"] - 3))
        merge(A, B, MaxTopNodes, sub, noB)
    elif B[noB]["Shift"] == A[noA]["Shift"]:
        A[noA]["Count"] += B[noB]["Count"]
        A[noA]["Cost"] += B[noB]["Cost"]
        if B[noB]["Daughter"] >= 0:
            for j in range(8):
                merge(A, B, MaxTopNodes, noA, B[noB]["Daughter"] + j)
        elif A[noA]["Daughter"] >= 0:
            for j in range(8):
                merge(A, B, MaxTopNodes, A[noA]["Daughter"] + j, noB)
    else:
        d = B[noB]["Shift"] - A[noA]["Shift"]
        if d > 60:
            return
        n = 1 << d
        A[noA]["Count"] += cdiv(B[noB]["Count"], n)
        A[noA]["Cost"] += cdiv(B[noB]["Cost"], n)
        if A[noA]["Daughter"] >= 0:
            for j in range(8):
                merge(A, B, MaxTopNodes, A[noA]["Daughter"] + j, noB)


# ---- domain_global_refine (:1320-1371), the copy (:469-476), domain_create_topleaves (:801-816) -------------------------------------
def global_refine(T, MaxTopNodes, countlimit, costlimit):
    i = 0
    while i < len(T):
        nd = T[i]
        if not (nd["Daughter"] >= 0 or nd["Shift"] <= 0) and not (nd["Count"] < countlimit and nd["Cost"] < costlimit):
            if len(T) + 8 > MaxTopNodes:
                return 1
            nd["Daughter"] = len(T)
            sh = nd["Shift"] - 3
            for j in range(8):
                T.append(new_node(nd["StartKey"] + j * (1 << sh), sh, -1, i, cdiv(nd["Count"], 8), cdiv(nd["Cost"], 8)))
        i += 1
    return 0


def finish(T, MaxTopNodes, countlimit, costlimit):
    """-> (TopNodes, TopLeaves) as structured arrays, or None when the refinement runs out of nodes.  T is refined in place."""
    if global_refine(T, MaxTopNodes, countlimit, costlimit):
        return None
    N = np.zeros(len(T), dtype=capi.TOPNODE_DTYPE)
    for f in ("StartKey", "Shift", "Daughter"):
        N[f] = [nd[f] for nd in T]
    N["Leaf"] = -1
    leaves = []

    def create(no):
        if N["Daughter"][no] == -1:
            N["Leaf"][no] = len(leaves)
            leaves.append(no)
        else:
            for j in range(8):
                create(int(N["Daughter"][no]) + j)
    create(0)
    L = np.zeros(len(leaves) + 1, dtype=capi.TOPLEAF_DTYPE)
    L["topnode"][:len(leaves)] = leaves
    return N, L


# ---- domain_assign_topleaves_balanced (:619-761), domain_set_task_leafs (:764-793), domain_check_memory_bound (:529-585) ----------------
def balance(N, L, cost, NTask, MaxPart, SetAsideFactor=1.0):
    """N, L: TopNodes / TopLeaves (ntopleaves + 1 entries) as finish() leaves them, changed in place; cost: TopLeafCount.
    -> (Tasks, status)"""
    ntl = len(L) - 1
    assert ntl >= NTask
    ext = [dict(topnode=int(L["topnode"][i]), Key=int(N["StartKey"][L["topnode"][i]]), Task=-1, cost=int(cost[i])) for i in range(ntl)]
    ext.sort(key=lambda e: e["Key"])
    totalcost = sum(e["cost"] for e in ext)
    left = totalcost
    Nsegment = NTask
    mean_expected = 1.0 * totalcost / Nsegment
    mean_task = 1.0 * totalcost / NTask
    curleaf = curseg = curtask = nrounds = 0
    curload = curtaskload = 0
    while nrounds < ntl:
        append = advance = 0
        if curleaf == ntl:
            advance = 1
        elif ntl - curleaf == Nsegment - curseg:
            append = advance = 1
        else:
            totalassigned = (totalcost - left) + curload
            if (mean_expected * (curseg + 1) - float(totalassigned) > 0.5 * ext[curleaf]["cost"]) or curload == 0:
                append = 1
            else:
                advance = 1
        if append:
            curload += ext[curleaf]["cost"]
            ext[curleaf]["Task"] = curtask
            curleaf += 1
        if advance:
            curtaskload += curload
            if (mean_task - float(curtaskload) < 0.5 * mean_expected) or (Nsegment - curseg <= NTask - curtask):
                curtaskload = 0
                curtask += 1
            left -= curload
            curload = 0
            curseg += 1
            if curtask == NTask:
                curtask = 0
                mean_expected = 1.0 * left / Nsegment
                mean_task = 1.0 * left / NTask
                nrounds += 1
            if curleaf == ntl:
                break
    assert curseg >= Nsegment and left == 0
    balance.nrounds = nrounds
    ext.sort(key=lambda e: (e["Task"], e["Key"]))
    for i, e in enumerate(ext):
        N["Leaf"][e["topnode"]] = i
        L["Task"][i] = e["Task"]
        L["topnode"][i] = e["topnode"]
    L["Task"][ntl] = NTask
    L["topnode"][ntl] = -1
    Tasks = np.zeros(NTask + 1, dtype=capi.TASK_LEAFS_DTYPE)
    ta = 0
    Tasks["StartLeaf"][0] = 0
    for i in range(ntl + 1):
        if L["Task"][i] == ta:
            continue
        Tasks["EndLeaf"][ta] = i
        ta += 1
        while ta < L["Task"][i]:
            Tasks["EndLeaf"][ta] = i
            Tasks["StartLeaf"][ta] = i
            ta += 1
        Tasks["StartLeaf"][ta] = i
    assert ta == NTask
    cost = np.asarray(cost, dtype=np.int64)
    max_load = max(int(cost[Tasks["StartLeaf"][t]:Tasks["EndLeaf"][t]].sum()) for t in range(NTask))
    return Tasks, int(max_load > MaxPart * SetAsideFactor)


def get_topleaf(N, keys):
    """domain_get_topleaf (domain.h:69-76) for an array of keys"""
    out = np.zeros(len(keys), dtype=np.int32)
    SK, D, S, Lf = (N[f].tolist() for f in ("StartKey", "Daughter", "Shift", "Leaf"))
    for i, k in enumerate(np.asarray(keys).tolist()):
        no = 0
        while D[no] >= 0:
            no = D[no] + ((k - SK[no]) >> (S[no] - 3))
        out[i] = Lf[no]
    return out


# ---- the policies (:378-403) ----------------------------------------------------------------------------------------------------
def policies(NTask, DomainOverDecompositionFactor):
    pol = []
    for i in range(NPOLICY):
        d = 256
        if i > 4 and pol[i - 1]["SubSampleDistance"] > 2:
            d = pol[i - 1]["SubSampleDistance"] // 2
        pol.append(dict(PreSort=int(i >= 2), SubSampleDistance=d, NTopLeaves=DomainOverDecompositionFactor * NTask * (i + 1)))
    return pol


# ---- domain_decompose_full for all ranks in one process ---------------------------------------------------------------------------
def combine_order(NTask):
    """(receiver, sender) pairs of domain_nonrecursively_combine_topTree (:1199-1250), in the order the merges happen on each receiver"""
    out = []
    sep = 1
    while sep < NTask:
        for r in range(0, NTask, 2 * sep):
            if r + sep < NTask:
                out.append((r, r + sep))
        sep *= 2
    return out


def decompose_serial(nxt, sub, ranks, box, params, policy_table=None):
    """ranks: per rank a dict(Pos [n][3], garbage bool [n], ID [n], MaxPart).  Runs the policy loop of :174-263 with every collective
    done in place.  -> dict(TopNodes, TopLeaves, Tasks, policy, factor, ids = per rank the sorted IDs it ends with, leaf_of = per rank
    (ID, TopLeaf) of what it ends with)"""
    NTask = len(ranks)
    pol = policy_table or policies(NTask, params["DomainOverDecompositionFactor"])
    factor = params["TopNodeAllocFactor"]
    keys = [PEANO(nxt, sub, r["Pos"], box) if len(r["Pos"]) else np.zeros(0, dtype=np.uint64) for r in ranks]
    for ip, p in enumerate(pol):
        while True:
            maxtop = [int(factor * (len(r["Pos"]) + 1)) for r in ranks]
            res = _attempt_serial(ranks, keys, p, maxtop)
            if res is not None:
                break
            factor *= 1.2
            if factor > 10:
                raise RuntimeError("TopNodeAllocFactor unreasonably large")
        N, L = res
        ntl = len(L) - 1
        assert ntl >= NTask
        count = np.zeros(ntl, dtype=np.int64)
        for r, k in zip(ranks, keys):
            live = ~np.asarray(r["garbage"], dtype=bool)
            count += np.bincount(get_topleaf(N, k[live]), minlength=ntl)
        Tasks, status = balance(N, L, count, NTask, ranks[0]["MaxPart"], params.get("SetAsideFactor", 1.0))
        if status and ip < len(pol) - 1:
            continue
        ids = [[] for _ in range(NTask)]
        for r, k in zip(ranks, keys):
            live = ~np.asarray(r["garbage"], dtype=bool)
            leaf = get_topleaf(N, k[live])
            for i, lf in zip(np.asarray(r["ID"])[live], leaf):
                ids[int(L["Task"][lf])].append((int(i), int(lf)))
        return dict(TopNodes=N, TopLeaves=L, Tasks=Tasks, policy=ip, factor=factor, leaf_of=[sorted(x) for x in ids],
                    ids=[sorted(i for i, _ in x) for x in ids])
    raise RuntimeError("no policy worked")


def _attempt_serial(ranks, keys, p, maxtop):
    NTask = len(ranks)
    local = [samples(k, r["garbage"], p["SubSampleDistance"], p["PreSort"]) for r, k in zip(ranks, keys)]
    allk = np.sort(np.concatenate(local), kind="stable")          # mpsort_mpi: globally sorted, every rank keeps as many as it gave
    off = np.concatenate([[0], np.cumsum([len(x) for x in local])])
    tot = len(allk)
    limit = tot // p["NTopLeaves"]
    trees = [local_toptree(allk[off[r]:off[r + 1]], limit, limit, maxtop[r]) for r in range(NTask)]
    if any(t is None for t in trees):
        return None
    err = False
    for recv, send in combine_order(NTask):
        if len(trees[recv]) + len(trees[send]) > maxtop[recv]:
            err = True
        else:
            merge(trees[recv], trees[send], maxtop[recv])
    T = trees[0]
    if err or any(len(T) >= m for m in maxtop):
        return None
    out = None
    for r in range(NTask):
        res = finish([dict(nd) for nd in T], maxtop[r], limit, limit)
        if res is None:
            return None
        out = res
    return out


# ---- the operators DistDomain drives, on the host ---------------------------------------------------------------------------------
class CpuDomainOps:
    """The `ops` of shenqi_amd.dist.DistDomain on numpy arrays through the procedures above: one rank's particles as Pos, garbage, ID,
    TopLeaf, and an exchange that sends whole rows through the communicator."""

    def __init__(self, nxt, sub, box, Pos, garbage, ID, MaxPart):
        self.nxt, self.sub, self.box = nxt, sub, box
        self.Pos = np.array(Pos, dtype=np.float64).reshape(-1, 3)
        self.garbage = np.array(garbage, dtype=bool)
        self.ID = np.array(ID, dtype=np.int64)
        self.TopLeaf = np.full(len(self.ID), -1, dtype=np.int32)
        self.MaxPart = MaxPart
        self.N = self.L = None

    @property
    def numpart(self):
        return len(self.ID)

    def _keys(self):
        return PEANO(self.nxt, self.sub, self.Pos, self.box) if len(self.Pos) else np.zeros(0, dtype=np.uint64)

    def samples(self, dist, presort):
        return samples(self._keys(), self.garbage, dist, presort)

    def local_toptree(self, lp, countlimit, costlimit, MaxTopNodes):
        T = local_toptree(lp, countlimit, costlimit, MaxTopNodes)
        return None if T is None else to_array(T)

    def merge(self, A, B, MaxTopNodes):
        TA = from_array(A)
        try:
            merge(TA, from_array(B), MaxTopNodes)
        except OutOfNodes:
            return None
        return to_array(TA)

    def finish(self, T, MaxTopNodes, countlimit, costlimit):
        return finish(from_array(T), MaxTopNodes, countlimit, costlimit)

    def balance(self, N, L, count, NTask, SetAsideFactor):
        return balance(N, L, count, NTask, self.MaxPart, SetAsideFactor)

    def install(self, N, L):
        self.N, self.L = N, L

    def leaf_counts(self):
        live = ~self.garbage
        return np.bincount(get_topleaf(self.N, self._keys()[live]), minlength=len(self.L) - 1).astype(np.int64)

    def particle_topleaves(self):
        live = ~self.garbage
        self.TopLeaf[live] = get_topleaf(self.N, self._keys()[live])
        target = np.full(self.numpart, -1, dtype=np.int32)
        target[live] = self.L["Task"][self.TopLeaf[live]]
        self.target = target
        return target

    def exchange(self, comm):
        """send every live particle to the task of its leaf; leavers and garbage are dropped here.  0, or 1 when MaxPart is passed"""
        import torch
        rows = np.concatenate([self.Pos, self.ID[:, None].astype(np.float64), self.TopLeaf[:, None].astype(np.float64)], axis=1)
        live = ~self.garbage
        stay = live & (self.target == comm.rank)
        order = np.argsort(self.target[live & ~stay], kind="stable")
        send = rows[live & ~stay][order]
        counts = np.bincount(self.target[live & ~stay], minlength=comm.size).tolist()
        recv, _ = comm.all_to_all_rows(torch.from_numpy(np.ascontiguousarray(send)), counts)
        rows = np.concatenate([rows[stay], recv.numpy().reshape(-1, 5)])
        self.Pos, self.ID, self.TopLeaf = rows[:, :3].copy(), rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int32)
        self.garbage = np.zeros(len(self.ID), dtype=bool)
        return int(len(self.ID) > self.MaxPart)

    def gc_sorted(self):
        k = self._keys()
        order = np.argsort(k, kind="stable")
        self.Pos, self.ID, self.TopLeaf, self.keys = self.Pos[order], self.ID[order], self.TopLeaf[order], k[order]


# ---- the positions whose keys the tests hold to the reference's PEANO() ------------------------------------------------------------------
KEY_BOXES = (4.0, 25000.0)


def key_positions(box):
    """4096 random positions, the corners 0 and Box (1 - 2^-52), and positions on, just below and just above exact cell boundaries of the
    2^21 grid PEANO() forms"""
    rng = np.random.default_rng(2021)
    top = box * (1.0 - 2.0 ** -52)
    fac = 1.0 / (box * 1.001) * (1 << BITS)
    m = rng.integers(1, int((1 << BITS) / 1.001) - 1, (256, 3)).astype(np.float64)
    edge = m / fac - box / 2000
    p = np.concatenate([rng.random((4096, 3)) * box, np.zeros((1, 3)), np.full((1, 3), top), [[0.0, top, 0.0]], edge, np.nextafter(edge, -np.inf),
                        np.nextafter(edge, np.inf)])
    return np.clip(p, 0.0, top)


def reference_PEANO(pos, box):
    """the reference's PEANO() of key_positions(box): from oracle/_ref where built, else the keys stored in tests/golden/ref_domain.npz"""
    lib = ro.peano_lib()
    if lib is not None:
        return np.array([lib.ref_PEANO(np.ascontiguousarray(p).ctypes.data, box) for p in np.asarray(pos, dtype=np.float64)], dtype=np.uint64)
    g = np.load(DOMAIN_GOLD)
    name = "box%g" % box
    assert str(g["fp_" + name]) == ro.fingerprint(pos, box), "positions differ from the stored ones: rerun tools/make_domain_golden.py"
    return g["key_" + name]


def domain_store():
    """what tests/golden/ref_domain.npz holds (tools/make_domain_golden.py): the tables derived from the reference's peano_hilbert_key and
    the reference's keys of key_positions()"""
    fn = reference_keyfn()
    assert fn is not None, "oracle/_ref/libpeano_ref.so missing: run `make -C oracle ref` first"
    nxt, sub = capi.peano_tables_to_arrays(capi.peano_tables_from_key(fn))
    out = {"next": nxt, "sub": sub}
    for box in KEY_BOXES:
        pos = key_positions(box)
        out["key_box%g" % box] = reference_PEANO(pos, box)
        out["fp_box%g" % box] = np.array(ro.fingerprint(pos, box))
    return out
