"""A numpy restatement of turn_on_quasars (libgadget/cooling_qso_lightup.cpp:489-596) for one rank, as the reference writes it: one draw
after another, each lit quasar ionising the not-yet-ionised gas inside its bubble (ionize_all_part's legacy walk, treewalk.c:905-1122,
as a vectorised mask over the gas), the HeIII fraction updated after each.  For a negative radius the walk's node test decides too: the
leaf of every candidate particle and all nodes above it are tested with cull_node on a host tree (sq.force_tree_rebuild_mask).  glibc's
log / cos / sqrt / pow are called through ctypes, as the reference's libm is.

No output of the reference itself is stored for this routine, so the restatement's parity with it rests on reading the code: it is the
yardstick of shq_heiii_reionization, not a pinned fixture."""
import ctypes as C
import math

import numpy as np

_libm = C.CDLL("libm.so.6")
for _f in ("log", "cos", "sqrt"):
    getattr(_libm, _f).argtypes = [C.c_double]
    getattr(_libm, _f).restype = C.c_double
_libm.pow.argtypes = [C.c_double, C.c_double]
_libm.pow.restype = C.c_double

# physconst.h, cooling_qso_lightup.cpp:48, treewalk.c:19
HYDROGEN_MASSFRAC = 0.76
PROTONMASS = 1.6726e-24
HEMASS = 4.002602
GAMMA_MINUS1 = 5.0 / 3.0 - 1
HUBBLE = 3.2407789e-18
GRAVITY = 6.672e-8
FACT1 = 0.366025403785
FLAG_GARBAGE, FLAG_HEIII = 1, 4


def nearest(x, box):
    """NEAREST (partmanager.h:99), elementwise"""
    return np.where(x > 0.5 * box, x - box, np.where(x < -0.5 * box, x + box, x))


def _nearest1(x, box):
    return x - box if x > 0.5 * box else (x + box if x < -0.5 * box else x)


def gaussian_rng(mu, sigma, seed, rnd):
    """gaussian_rng (:249-255): Box-Muller on Table[seed % size], Table[(seed + 1) % size]"""
    u1 = rnd[seed % len(rnd)]
    u2 = rnd[(seed + 1) % len(rnd)]
    z1 = _libm.sqrt(-2 * _libm.log(u1)) * _libm.cos(2 * math.pi * u2)
    return mu + sigma * z1


def cull_node(node, cm, R, box):
    """cull_node (treewalk.c:990-1019), asymmetric: 1 if the walk opens the node"""
    dist = R + 0.5 * float(node["len"])
    r2 = 0.0
    for d in range(3):
        dx = _nearest1(float(node["center"][d]) - cm[d], box)
        if dx > dist:
            return False
        if dx < -dist:
            return False
        r2 += dx * dx
    dist += FACT1 * float(node["len"])
    return not (r2 > dist * dist)


def walk_reaches(p, cm, R, tree, box):
    """the walk from the root reaches particle p's leaf only if the leaf and every node above it pass cull_node"""
    nodes, first, father = tree
    no = int(father[p])
    if no < first:
        return False
    while no >= 0:
        rec = nodes[no - first]
        if not cull_node(rec, cm, R, box):
            return False
        no = int(rec["father"])
    return True


def host_tree(t, numpart):
    """(Nodes_base, firstnode, Father) of a sq.ForceTree"""
    v = t.view()
    father = np.ctypeslib.as_array((C.c_int32 * numpart).from_address(v.father)).copy()
    return t.Nodes_base.copy(), t.firstnode, father


def _heat(idx, flags, entropy, pi, density, a3inv, deltau, uu):
    """ionize_single_particle (:354-373) for particles that are not ionised yet"""
    flags[idx] |= FLAG_HEIII
    for i in idx:
        s = pi[i]
        entropytou = _libm.pow(float(density[s]) * a3inv, GAMMA_MINUS1) / GAMMA_MINUS1
        entropy[s] += deltau / uu / entropytou


def turn_on_quasars(pos, types, flags, pi, density, entropy, groups, rnd, P, tree=None, stop_after=None):
    """P: dict of shq_heiii_params' fields.  groups: the catalogue (FOF_GROUP_DTYPE: Mass, MinID, CM), TotNgroups = len(groups).
    tree: host_tree(...) of the gas tree, needed when a radius is negative.  Returns (flags, entropy, log, result): the updated copies,
    the FdHelium lines as (group, pos[3], ionfrac, n_ionized) tuples (group -1 and zeros when no halo was walked), and a dict of
    shq_heiii_result's fields.  stop_after: end the loop after that many iterations (a probe of the trajectory, not the reference)."""
    flags = np.array(flags, dtype=np.uint8, copy=True)
    entropy = np.array(entropy, dtype=np.float64, copy=True)
    box = P["BoxSize"]
    n_gas_tot = int(P["n_gas_tot"])
    a3inv = 1 / _libm.pow(P["atime"], 3)
    nheperg = (1 - HYDROGEN_MASSFRAC) / (PROTONMASS * HEMASS)
    deltau = P["qso_inst_heating"] * nheperg
    uu = P["uu_in_cgs"]
    desired = P["desired_ion_frac"]
    gas = types == 0
    res = dict(init_ionfrac=0.0, final_ionfrac=0.0, n_candidates=0, n_iterations=0, n_flash=0, n_ionized=0)
    # flash (:501-512): every Type-0 particle below NumPart, garbage included
    if desired > P["heIIIreion_finish_frac"]:
        idx = np.flatnonzero(gas & ((flags & FLAG_HEIII) == 0))
        _heat(idx, flags, entropy, pi, density, a3inv, deltau, uu)
        res["n_flash"] = len(idx)
    rhobar = P["OmegaBaryon"] * (3 * HUBBLE * P["HubbleParam"] * HUBBLE * P["HubbleParam"]) / (8 * math.pi * GRAVITY) * a3inv
    totbubblegasmass = 4 * math.pi / 3. * _libm.pow(P["mean_bubble"], 3) * rhobar
    non_overlapping_bubble_number = int(n_gas_tot * totbubblegasmass / P["OmegaBaryon"])
    initionfrac = int(np.count_nonzero(gas & ((flags & FLAG_HEIII) != 0))) / n_gas_tot
    cur = initionfrac
    res["init_ionfrac"] = res["final_ionfrac"] = initionfrac
    qso_cand = []
    if cur < desired:   # build_qso_candidate_list (:260-276)
        qso_cand = [g for g in range(len(groups))
                    if not (groups["Mass"][g] < P["qso_candidate_min_mass"]) and not (groups["Mass"][g] > P["qso_candidate_max_mass"])]
    res["n_candidates"] = len(qso_cand)
    log = []
    if not qso_cand:
        return flags, entropy, log, res
    ncand_tot, ncand_before = len(qso_cand), 0
    sigma = _libm.sqrt(P["var_bubble"])
    tot = 0
    iteration = 0
    while cur < desired and (stop_after is None or iteration < stop_after):
        # choose_QSO_halo (:314-328)
        drand = rnd[(len(groups) + iteration) % len(rnd)]
        qso = int(drand * ncand_tot)
        ncand_tot -= 1
        if qso < ncand_before:
            ncand_before -= 1
        new_qso = -1 if (qso < ncand_before or qso >= ncand_before + len(qso_cand)) else qso - ncand_before
        if ncand_tot <= 0:
            break
        n_ionized = 0
        qpos = (0.0, 0.0, 0.0)
        group = -1
        if new_qso > 0:   # ionize_all_part walks only for qso_ind > 0
            group = qso_cand[new_qso]
            cm = [float(x) for x in groups["CM"][group]]
            R = gaussian_rng(P["mean_bubble"], sigma, int(groups["MinID"][group]), rnd)
            with np.errstate(invalid="ignore", over="ignore"):
                dx = nearest(cm[0] - pos[:, 0], box)
                dy = nearest(cm[1] - pos[:, 1], box)
                dz = nearest(cm[2] - pos[:, 2], box)
                r2 = dx * dx
                r2 = r2 + dy * dy
                r2 = r2 + dz * dz
                inside = ~(r2 > R * R)
            sel = gas & ((flags & (FLAG_GARBAGE | FLAG_HEIII)) == 0) & inside
            idx = np.flatnonzero(sel)
            if R < 0:
                if tree is None:
                    raise ValueError("a negative radius needs the gas tree")
                idx = np.array([i for i in idx if walk_reaches(i, cm, R, tree, box)], dtype=np.int64)
            _heat(idx, flags, entropy, pi, density, a3inv, deltau, uu)
            n_ionized = len(idx)
            qp = []
            for d in range(3):
                x = cm[d] - P["CurrentParticleOffset"][d]
                if math.isfinite(x):
                    while x > box:
                        x -= box
                    while x <= 0:
                        x += box
                qp.append(x)
            qpos = tuple(qp)
        cur += n_ionized / n_gas_tot
        tot += n_ionized
        log.append((group, qpos, cur, n_ionized))
        if n_ionized < 0.01 * non_overlapping_bubble_number and iteration > 10:
            break
        if new_qso >= 0:
            del qso_cand[new_qso]
        iteration += 1
    res.update(final_ionfrac=cur, n_iterations=len(log), n_ionized=tot)
    return flags, entropy, log, res
