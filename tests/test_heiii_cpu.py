"""The restatement of turn_on_quasars (heiii_restated.py) on hand-built random tables: the reference's quirks that the device call has to
reproduce — a position-0 draw walks nothing, the last candidate is never lit, u1 = 0 takes every eligible gas particle, a negative radius
lets the tree decide, the flash takes garbage gas, bubbles skip garbage and converted (Type 5) particles.  CPU only."""
import numpy as np

import shenqi_amd as sq
from shenqi_amd import capi
import heiii_restated as hr

BOX = 20000.0
NRND = 64


def params(**kw):
    p = dict(BoxSize=BOX, atime=0.25, qso_candidate_min_mass=1.0, qso_candidate_max_mass=100.0, mean_bubble=3000.0, var_bubble=0.0,
             heIIIreion_finish_frac=0.95, desired_ion_frac=0.9, qso_inst_heating=2e-12, uu_in_cgs=1e10, OmegaBaryon=0.045, HubbleParam=0.7,
             CurrentParticleOffset=(0.0, 0.0, 0.0), n_gas_tot=0)
    p.update(kw)
    return p


def particles(ngas=600, ndm=200, seed=3):
    """uniform gas and dark matter; a few gas particles are garbage, a few converted to Type 5"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, BOX, (ngas + ndm, 3))
    types = np.concatenate([np.zeros(ngas, np.uint8), np.ones(ndm, np.uint8)])
    types[rng.choice(ngas, 10, replace=False)] = 5
    flags = np.zeros(ngas + ndm, np.uint8)
    gas = np.flatnonzero(types == 0)
    flags[gas[:12]] |= hr.FLAG_GARBAGE
    flags[gas[12:20]] |= hr.FLAG_HEIII | 8      # already ionised (and BHHeated)
    pi = np.full(ngas + ndm, -1, np.int32)
    pi[:ngas] = np.arange(ngas)                  # Type 5 keeps its old gas slot here: never read
    density = rng.uniform(0.5, 2.0, ngas)
    entropy = rng.uniform(1.0, 3.0, ngas)
    return pos, types, flags, pi, density, entropy


def groups(cms, masses, minids):
    g = np.zeros(len(cms), dtype=capi.FOF_GROUP_DTYPE)
    g["CM"], g["Mass"], g["MinID"] = cms, masses, minids
    return g


def table(entries):
    rnd = np.full(NRND, 0.5)
    for k, v in entries.items():
        rnd[k] = v
    return rnd


def run(rnd, grp, tree=None, ps=None, **kw):
    pos, types, flags, pi, density, entropy = ps if ps is not None else particles()
    p = params(n_gas_tot=int(np.count_nonzero(types == 0)), **kw)
    return hr.turn_on_quasars(pos, types, flags, pi, density, entropy, grp, rnd, p, tree), (pos, types, flags, pi, density, entropy)


# four candidates; the draws read Table[4 + t]: position 0 (group 0 erased), then positions of groups 2 and 3, then the list runs out
FOUR = groups([[5000, 5000, 5000], [15000, 5000, 5000], [5000, 15000, 5000], [5000, 5000, 15000]], [10, 20, 30, 40], [20, 22, 24, 26])
SEQ = {4: 0.0, 5: 0.5, 6: 0.9, 7: 0.1, 20: 0.3, 21: 0.1, 22: 0.3, 23: 0.1, 24: 0.3, 25: 0.1, 26: 0.3, 27: 0.1}


def test_position_zero_draw_walks_nothing_and_logs_zeros():
    (flags, _, log, res), _ = run(table(SEQ), FOUR)
    assert res["n_candidates"] == 4
    group, pos, frac, nion = log[0]
    assert group == -1 and pos == (0.0, 0.0, 0.0) and nion == 0 and frac == res["init_ionfrac"]
    assert [g for g, *_ in log] == [-1, 2, 3]           # group 0 was erased by the position-0 draw
    assert all(n > 0 for *_, n in log[1:])


def test_last_candidate_is_never_lit():
    (_, _, log, res), _ = run(table(SEQ), FOUR)
    assert res["n_iterations"] == 3 and 1 not in [g for g, *_ in log]
    assert res["final_ionfrac"] < 0.9                    # the target was not reached: the list ran out
    one = groups([[5000, 5000, 5000]], [10], [20])
    (_, _, log1, res1), _ = run(table(SEQ), one)
    assert res1["n_candidates"] == 1 and res1["n_iterations"] == 0 and log1 == []


def test_zero_u1_takes_every_eligible_gas_particle():
    seq = dict(SEQ)
    seq[24] = 0.0                                         # group 2's u1: sqrt(-2 log 0) = inf, times 0 (var = 0) = NaN
    (flags, _, log, res), (_, types, flags0, *_) = run(table(seq), FOUR)
    eligible = (types == 0) & ((flags0 & (hr.FLAG_GARBAGE | hr.FLAG_HEIII)) == 0)
    assert log[1][0] == 2 and log[1][3] == int(eligible.sum())
    assert np.all(flags[eligible] & hr.FLAG_HEIII)
    assert len(log) == 2 and res["final_ionfrac"] >= 0.9  # the target is reached with it


def test_garbage_and_converted_gas_skipped_by_bubbles_flashed_when_gas():
    seq = dict(SEQ)
    seq[24] = 0.0
    (flags, entropy, _, _), (_, types, flags0, pi, _, entropy0) = run(table(seq), FOUR)
    garbage = (types == 0) & (flags0 & hr.FLAG_GARBAGE != 0)
    assert not np.any(flags[garbage] & hr.FLAG_HEIII) and np.array_equal(entropy[pi[garbage]], entropy0[pi[garbage]])
    assert not np.any(flags[types == 5] & hr.FLAG_HEIII) and not np.any(flags[types == 1] & hr.FLAG_HEIII)
    # the flash: every Type-0 particle, garbage included, nothing of another type; other flag bits kept
    (ff, fe, flog, fres), _ = run(table(SEQ), FOUR, desired_ion_frac=0.97)
    gas = types == 0
    fresh = gas & (flags0 & hr.FLAG_HEIII == 0)
    assert fres["n_flash"] == int(fresh.sum()) and np.all(ff[gas] & hr.FLAG_HEIII) and not np.any(ff[~gas] & hr.FLAG_HEIII)
    assert np.all(fe[pi[garbage]] > entropy0[pi[garbage]])
    assert np.array_equal(ff & ~np.uint8(hr.FLAG_HEIII), flags0 & ~np.uint8(hr.FLAG_HEIII))
    assert fres["init_ionfrac"] == 1.0 and fres["n_candidates"] == 0 and flog == []


def test_negative_radius_lets_the_tree_decide():
    """R < 0 (var > 0): the particle test alone takes the gas within |R| of the centre, the walk opens only nodes that pass cull_node
    with the negative radius — the whole ball must lie inside the particle's leaf.  A ball across a leaf boundary ionises nothing, a
    ball inside one leaf ionises what the particle test takes."""
    ps = particles(ngas=300, ndm=50, seed=5)
    pos, types, flags0 = ps[0], ps[1], ps[2]
    pman = sq.PartManager(len(pos), BOX)
    pman.Base["Pos"], pman.Base["Type"], pman.Base["Mass"] = pos, types, 1.0
    t = sq.force_tree_rebuild_mask(pman, sq.GASMASK | sq.BHMASK)
    tree = hr.host_tree(t, len(pos))
    nodes, first, father = tree
    eligible = (types == 0) & ((flags0 & (hr.FLAG_GARBAGE | hr.FLAG_HEIII)) == 0)
    # a gas particle deep inside its leaf, and one right next to a face of its leaf
    depth = []
    for i in np.flatnonzero(eligible):
        leaf = nodes[father[i] - first]
        depth.append((0.5 * leaf["len"] - np.abs(pos[i] - leaf["center"]).max(), i))
    depth.sort()
    deep, shallow = depth[-1][1], depth[0][1]
    for i, R, taken in ((deep, -40.0, True), (shallow, -1.0 - depth[0][0], False)):
        cm = pos[i] + [0.25 * abs(R), 0.0, 0.0]
        grp = FOUR.copy()
        grp["CM"][2] = cm
        seq = dict(SEQ)
        seq[24], seq[25] = 0.5, 0.25                      # cos(pi / 2) ~ 6e-17: R = mean + sigma z1 ~ mean
        (flags, _, log, _), _ = run(table(seq), grp, tree=tree, ps=ps, mean_bubble=R, var_bubble=1e-6)
        d = hr.nearest(cm[None, :] - pos, BOX)
        inside = eligible & ~((d ** 2).sum(1) > R * R)
        assert log[1][0] == 2 and inside[i]
        assert log[1][3] == (int(inside.sum()) if taken else 0), (i, R, log[1], int(inside.sum()))
    # the particle test alone (no tree) is what a positive radius of the same size takes
    (_, _, logp, _), _ = run(table(seq), grp, ps=ps, mean_bubble=-R, var_bubble=0.0)
    assert logp[1][3] == int(inside.sum()) > 0
