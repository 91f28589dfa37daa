"""All-pairs restatement of the two black-hole walks of csrc/sph_bh.hip (libgadget/blackhole.cpp:373-965: accretion ngbiter and
postprocess, feedback ngbiter, haswork and postprocess) in np.longdouble.  No tree, no oracle/blackhole.py, plain numpy, in the
manner of ngbsums_brute.py, whose kernel values are reused.

Conventions:
  - a hole's neighbours are ALL particles that were put into the tree when it was built (`in_tree`), are no garbage NOW and are gas
    or a hole NOW, with r2 <= max(Hsml_i, Hsml_j)^2 (treewalk_visit_ngbiter, treewalk.c:925-975, symmetric).  The Swallowed flag is
    not looked at: a hole that was swallowed after the build is a neighbour, as in the reference's text (its tree build leaves
    swallowed holes out, forcetree.cpp:805, its walk does not);
  - the separation is the minimum image `d - Box * round(d / Box)` in f64 and every distance test is taken on the f64
    r2 = (d0^2 + d1^2) + d2^2; pair terms are formed and added in np.longdouble and rounded to f64 once; the decisions of the
    postprocess are taken on the long-double values, and every decision records how far it was from its threshold (`margins`);
  - every floating-point output comes with a per-element SCALE: the sum of the absolute values of the terms that formed it,
    carried through the postprocess formulas to first order (a quotient or product adds the relative scales of its factors, a
    kernel value counts with the absolute values of its polynomial's terms).  An element nothing wrote has scale 0 and must
    keep its bits;
  - the marks on the neighbours' side are returned as the list the emit / resolve / apply route emits, (row, queue position, kind,
    ID) and (row, queue position, kind, value), and resolved here: a gas particle keeps the largest ID + 1, a hole the result of
    the reference's compare-and-swap rule (blackhole.cpp:546-560).  That rule is applied in queue order, in reverse order and in
    three seeded random orders, and the results must agree: they do as long as no two hole IDs are consecutive (the rule compares
    a mark, ID + 1, with an ID);
  - the heat a gas particle receives is applied as min(u0 + sum, MaxThermalU): every injection is positive and the clamp is
    monotone, so the arrival order does not matter;
  - `tally` counts every branch by the names of BRANCHES below; each `if` of the pair lambdas and postprocess kernels of
    sph_bh.hip has a name for either side.
The kernels' task loop with more tasks than workgroups (more than 262 144 holes in a queue) is not reachable at test sizes.
"""
from types import SimpleNamespace

import numpy as np

from density_brute import LD, min_image
from ngbsums_brute import wk_values

GAMMA = LD(5) / 3
GAMMA_MINUS1 = GAMMA - 1
TIMEBINS = 46
PI = LD("3.14159265358979323846264338327950288")

ACC_PAIR = ("mass_negative", "wind_decoupled", "self", "bh_no_record", "bh_far", "bh_near_no_neighbour", "encounter", "flag_reposition", "flag_nobound",
            "bound_yes", "bound_no", "gas_outside_kernel", "gas_inside_kernel", "seed_off", "seed_below", "seed_reached", "pacc_no_excess",
            "pacc_no_density", "pacc_positive", "draw_hit", "draw_miss", "mgas_on", "mgas_off", "no_neighbour",
            "timebin_active", "timebin_inactive", "timebin_bin0", "timebin_ti0",
            "cas_first_larger_id", "cas_first_inactive", "cas_replace", "cas_keep", "mark_first", "mark_raised", "mark_kept")
ACC_POST = ("density_positive", "density_zero", "norm_positive", "norm_zero", "edd_capped", "edd_free", "edd_off", "drag0", "drag1", "drag2",
            "ke_off", "ke_low_x", "ke_low_thr", "ke_accumulate", "ke_high", "eps_capped", "eps_free", "ke_release", "ke_hold", "vdisp_zero")
FB_PAIR = ("fb_no_work", "fb_self", "fb_wind_decoupled", "bh_unmarked", "bh_marked_elsewhere", "bh_swallowed", "fb_bh_no_record", "othermass_seed_off",
           "othermass_imtrack_zero", "othermass_mtrack", "othermass_particle", "fb_other_type", "gas_unmarked_inside", "gas_unmarked_outside",
           "mintimebin_lowered", "mintimebin_kept", "heat", "heat_no_weight", "heat_no_energy", "heat_kinetic_channel", "heat_zero_mass",
           "eeqos_flagged", "eeqos_not", "eeqos_absent", "heat_capped", "heat_capped_by_one", "heat_capped_by_sum", "heat_free",
           "kick", "kick_no_density", "kick_nothing_released", "kick_thermal_channel", "gas_marked_elsewhere", "gas_swallowed",
           "channel_thermal", "channel_kinetic_hold", "channel_kinetic_release")
FB_POST = ("bhmass_grows", "bhmass_kept", "bhmass_only", "mass_nothing", "mtrack_grows", "mtrack_saturates", "mass_grows", "ke_reset", "ke_kept")
BRANCHES = ACC_PAIR + ACC_POST + FB_PAIR + FB_POST
MARGINS = ("ngb_radius", "rmerge", "kernel", "bound", "draw", "excess", "seed", "seed_sum", "eddington", "edd_ratio", "lam_x", "epsilon",
           "ke_thresh", "max_u")


def _note(margins, name, values):
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    if values.size:
        margins[name] = min(margins.get(name, np.inf), float(values.min()))


def _dist(a, b, sa, sb):
    """|a - b| relative to the larger of the two scales"""
    s = max(float(sa), float(sb))
    return abs(float(a - b)) / s if s > 0 else np.inf


def kicks(kf):
    return SimpleNamespace(g=np.array(kf.gravkicks[:], dtype=np.float64), h=np.array(kf.hydrokicks[:], dtype=np.float64),
                           dloga=np.array(kf.dloga_for_bin[:], dtype=np.float64), FB=float(kf.FgravkickB))


def timebin_active(b, cur):
    """is_timebin_active, timestep.cpp:132-139"""
    if b <= 0 or cur <= 0:
        return True
    return cur % (1 << int(b)) == 0


def velpred(P, S, k, rows, gas):
    """DM_VelPred / SPH_VelPred (density2.h:89-111) of `rows` in long double with the sum of the absolute values of its terms"""
    v, a, pm = (P[x][rows].astype(LD) for x in ("Vel", "FullTreeGravAccel", "GravPM"))
    gk = k.g[P["TimeBinGravity"][rows].astype(np.int64)].astype(LD)[:, None]
    val, sc = v + gk * a + pm * LD(k.FB), np.abs(v) + np.abs(gk * a) + np.abs(pm * LD(k.FB))
    if gas:
        hk = k.h[P["TimeBinHydro"][rows].astype(np.int64)].astype(LD)[:, None]
        ha = S["HydroAccel"][P["PI"][rows].astype(np.int64)].astype(LD)
        val, sc = val + hk * ha, sc + np.abs(hk * ha)
    return val, sc


class _Set:
    """what both walks need of a particle set: the candidates, and per hole the f64 distances to them"""

    def __init__(self, P, S, ids, prm, in_tree):
        self.P, self.S, self.ids, self.prm = P, S, np.asarray(ids, dtype=np.uint64), prm
        self.box = float(prm.BoxSize)
        t, f = P["Type"], P["Flags"]
        self.cand = np.flatnonzero(np.asarray(in_tree, dtype=bool) & ((f & 1) == 0) & ((t == 0) | (t == 5)))
        c = self.cand
        self.ctype, self.cpi, self.chs, self.cid = t[c], P["PI"][c].astype(np.int64), P["Hsml"][c], self.ids[c]
        self.cmass = P["Mass"][c].astype(np.float64)
        self.isgas, self.ishole = self.ctype == 0, self.ctype == 5
        self.delayed = np.zeros(len(c), dtype=bool)
        if prm.WindsDecoupleSph:
            self.delayed[self.isgas] = S["DelayTime"][self.cpi[self.isgas]] > 0

    def around(self, i, margins):
        """(d, r2, accepted) of hole i to every candidate, the neighbour test of the walk"""
        P, c = self.P, self.cand
        d = min_image(P["Pos"][i][None, :] - P["Pos"][c], self.box)
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        hm = np.maximum(P["Hsml"][i], self.chs)
        _note(margins, "ngb_radius", np.abs(r2 / (hm * hm) - 1))
        H = P["Hsml"][i]
        _note(margins, "kernel", np.abs(r2[self.isgas] / (H * H) - 1))
        return d, r2, r2 <= hm * hm


def resolve_marks(marks, order, P, ids, Ti_Current, nsph, nbh, tally=None):
    """the two mark rules over `marks` = [(row, queue position, kind, ID)] taken in `order`: (SPH_SwallowID, BH_SwallowID) by slot"""
    sph, bh = np.zeros(nsph, dtype=np.uint64), np.zeros(nbh, dtype=np.uint64)
    for k in order:
        row, _, kind, myid = marks[k]
        slot, myid = int(P["PI"][row]), int(myid)
        if kind == 1:
            old = int(sph[slot])
            if old < myid + 1:
                sph[slot] = myid + 1
            if tally is not None:
                tally["mark_first" if old == 0 else "mark_raised" if old < myid + 1 else "mark_kept"] += 1
            continue
        readid, oid, b = int(bh[slot]), int(ids[row]), int(P["TimeBinHydro"][row])
        active = timebin_active(b, Ti_Current)
        if readid != 0 and readid < myid:
            bh[slot], name = myid + 1, "cas_replace"
        elif readid == 0 and (oid < myid or not active):
            bh[slot], name = myid + 1, "cas_first_larger_id" if oid < myid else "cas_first_inactive"
        else:
            name = "cas_keep"
        if tally is not None:
            tally[name] += 1
            tally["timebin_bin0" if b <= 0 else "timebin_ti0" if Ti_Current <= 0 else "timebin_active" if active else "timebin_inactive"] += 1
    return sph, bh


def mark_orders(marks, P, ids, Ti_Current, nsph, nbh, tally):
    """the marks in queue order, and whether the reverse and three random orders end in the same marks"""
    fwd = sorted(range(len(marks)), key=lambda k: (marks[k][1], marks[k][0]))
    sph, bh = resolve_marks(marks, fwd, P, ids, Ti_Current, nsph, nbh, tally)
    same = True
    for order in [fwd[::-1]] + [list(np.random.default_rng(s).permutation(len(marks))) for s in (1, 2, 3)]:
        s2, b2 = resolve_marks(marks, order, P, ids, Ti_Current, nsph, nbh)
        same = same and np.array_equal(s2, sph) and np.array_equal(b2, bh)
    return sph, bh, same


def new_work(nsph, nbh, sentinel=0.0):
    return dict(SPH_SwallowID=np.full(nsph, 99, dtype=np.uint64), BH_SwallowID=np.full(nbh, 99, dtype=np.uint64),
                BH_FeedbackWeightSum=np.full(nbh, sentinel), BH_Entropy=np.full(nbh, sentinel), BH_SurroundingGasVel=np.full((nbh, 3), sentinel),
                MgasEnc=np.full(nbh, sentinel), KEflag=np.zeros(nbh, dtype=np.int32), BH_accreted_Mass=np.full(nbh, sentinel),
                BH_accreted_BHMass=np.full(nbh, sentinel), BH_accreted_momentum=np.full((nbh, 3), sentinel))


def _scales(P, S, B, work):
    sc = {"P.Vel": np.zeros((len(P), 3)), "P.Mass": np.zeros(len(P)), "S.Entropy": np.zeros(len(S))}
    for k in ("Mdot", "Mass", "Mtrack", "KineticFdbkEnergy"):
        sc["B." + k] = np.zeros(len(B))
    sc["B.DragAccel"] = np.zeros((len(B), 3))
    for k, v in work.items():
        if v.dtype == np.float64:
            sc["work." + k] = np.zeros(v.shape)
    return sc


def accretion(P, S, B, ids, queue, kf, prm, Ti_Current, rnd, in_tree, work):
    """treewalk_run(tw_accretion) for the holes `queue` on copies of the records and of `work`.  Returns a namespace: P, S, B, work
    after the walk, scale (name -> array, see the module text), marks [(row, queue position, kind, ID)], tally, margins,
    marks_order_free, nngb (accepted neighbours per queue position)."""
    P, S, B, work = P.copy(), S.copy(), B.copy(), {k: v.copy() for k, v in work.items()}
    ids = np.asarray(ids, dtype=np.uint64)
    k, kt, n = kicks(kf), prm.DensityKernelType, len(P)
    Z = _Set(P, S, ids, prm, in_tree)
    tally, margins, marks = dict.fromkeys(BRANCHES, 0), {}, []
    sc = _scales(P, S, B, work)
    rmerge = 2 * prm.ForceSoftening / 2.8
    nrnd = np.uint64(len(rnd))
    gas_rows = Z.cand[Z.isgas]
    vp_gas, vps_gas = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    if len(gas_rows):
        vp_gas[gas_rows], vps_gas[gas_rows] = velpred(P, S, k, gas_rows, True)
    hole_rows = Z.cand[Z.ishole]
    vp_bh = np.zeros((n, 3), dtype=LD)
    if len(hole_rows):
        vp_bh[hole_rows] = velpred(P, S, k, hole_rows, False)[0]
    work["SPH_SwallowID"][:] = 0                                       # blackhole.cpp:270-274
    work["BH_SwallowID"][:] = 0
    nngb = np.zeros(len(queue), dtype=np.int64)
    post = []
    for t, i in enumerate(queue):
        i = int(i)
        b = int(P["PI"][i])
        myid = ids[i]
        h = float(P["Hsml"][i])
        imass, ibh, idens, imtrack = LD(P["Mass"][i]), LD(B["Mass"][b]), LD(B["Density"][b]), LD(B["Mtrack"][b])
        d, r2, acc = Z.around(i, margins)
        near_out = Z.ishole & ~acc & (np.sqrt(r2) < rmerge) & (Z.cid != myid)
        tally["bh_near_no_neighbour"] += int(near_out.sum())
        nngb[t] = int(acc.sum())
        if nngb[t] == 0 or (nngb[t] == 1 and Z.cid[acc][0] == myid):
            tally["no_neighbour"] += 1
        neg = acc & (Z.cmass < 0)
        dec = acc & ~neg & Z.delayed
        me = acc & ~neg & ~dec & (Z.cid == myid)
        rest = acc & ~neg & ~dec & ~me
        tally["mass_negative"] += int(neg.sum())
        tally["wind_decoupled"] += int(dec.sum())
        tally["self"] += int(me.sum())
        # ---- holes
        r = np.sqrt(r2)
        holes = np.flatnonzero(rest & Z.ishole)
        _note(margins, "rmerge", np.abs(r[holes] / rmerge - 1))
        enc = 0
        iacc = P["FullTreeGravAccel"][i].astype(LD) + P["GravPM"][i].astype(LD) + B["DFAccel"][b].astype(LD)
        for j in holes:
            if not r[j] < rmerge:
                tally["bh_far"] += 1
                continue
            tally["encounter"] += 1
            enc = 1
            o = int(Z.cand[j])
            flag = 0
            if prm.RepositionEnabled == 1:
                flag = 1
                tally["flag_reposition"] += 1
            if prm.MergeGravBound == 0:
                flag = 1
                tally["flag_nobound"] += 1
            if prm.MergeGravBound == 1 and prm.RepositionEnabled == 0:       # check_grav_bound, :160-180
                dv = P["Vel"][i].astype(LD) - vp_bh[o]
                da = iacc - P["FullTreeGravAccel"][o].astype(LD) - P["GravPM"][o].astype(LD) - B["DFAccel"][Z.cpi[j]].astype(LD)
                dx = d[j].astype(LD)
                KE = (0.5 * dv * dv).sum() / (LD(prm.atime) * LD(prm.atime))
                PE, aPE = (da * dx).sum() / LD(prm.atime), np.abs(da * dx).sum() / LD(prm.atime)
                _note(margins, "bound", abs(float(PE + KE)) / float(aPE + KE) if aPE + KE > 0 else np.inf)
                flag = 1 if PE + KE <= 0 else 0
                tally["bound_yes" if flag else "bound_no"] += 1
            if flag == 1:
                marks.append((o, t, 0, int(myid)))
        # ---- gas
        H = LD(h)
        gas = rest & Z.isgas
        ins = np.flatnonzero(gas & (r2 < h * h))
        tally["gas_outside_kernel"] += int(gas.sum()) - len(ins)
        tally["gas_inside_kernel"] += len(ins)
        rows = Z.cand[ins]
        dl = d[ins].astype(LD)
        rl = np.sqrt((dl * dl).sum(axis=1))
        wk, wka = wk_values(kt, H, rl), wk_values(kt, H, rl, True)
        mj = Z.cmass[ins].astype(LD)
        ent = S["Entropy"][Z.cpi[ins]].astype(LD)
        fws, sfws = (mj * wk).sum(), (mj * wka).sum()
        sment, ssment = (mj * wk * ent).sum(), (mj * wka * np.abs(ent)).sum()
        gv, sgv = (mj * wk)[:, None] * vp_gas[rows], (mj * wka)[:, None] * vps_gas[rows]
        gv, sgv = gv.sum(axis=0) if len(ins) else np.zeros(3, dtype=LD), sgv.sum(axis=0) if len(ins) else np.zeros(3, dtype=LD)
        seed = LD(prm.SeedBHDynMass)
        part = imass
        if seed > 0:
            _note(margins, "seed", abs(float(imtrack / seed - 1)))
        if seed > 0 and imtrack < seed:
            part = imtrack
            tally["seed_below"] += 1
        else:
            tally["seed_reached" if seed > 0 else "seed_off"] += 1
        _note(margins, "excess", _dist(ibh, part, abs(ibh), abs(part)))
        pacc, paccs = np.zeros(len(ins), dtype=LD), np.zeros(len(ins), dtype=LD)
        if (ibh - part) > 0 and idens > 0:
            pacc, paccs = (ibh - part) * wk / idens, (abs(ibh) + abs(part)) * wka / idens
            tally["pacc_positive"] += len(ins)
        else:
            tally["pacc_no_excess" if not (ibh - part) > 0 else "pacc_no_density"] += len(ins)
        rn = np.asarray(rnd, dtype=np.float64)[(Z.cid[ins] % nrnd).astype(np.int64)].astype(LD)
        hit = rn < pacc
        _note(margins, "draw", (np.abs(rn - pacc) / np.maximum(np.maximum(paccs, rn), LD(1e-300))).astype(np.float64))
        tally["draw_hit"] += int(hit.sum())
        tally["draw_miss"] += int((~hit).sum())
        marks.extend((int(o), t, 1, int(myid)) for o in rows[hit])
        mgas = mj.sum() if prm.BlackHoleKineticOn == 1 else LD(0)
        tally["mgas_on" if prm.BlackHoleKineticOn == 1 else "mgas_off"] += len(ins)
        post.append((i, b, enc, fws, sfws, sment, ssment, gv, sgv, mgas))
    nsph, nbh = len(S), len(B)
    sph, bhm, same = mark_orders(marks, P, ids, Ti_Current, nsph, nbh, tally)
    assert same, "the hole marks depend on the order the candidates arrive in: are two hole IDs consecutive?"
    work["SPH_SwallowID"][:], work["BH_SwallowID"][:] = sph, bhm
    for rec in post:
        _accretion_post(P, B, k, prm, work, sc, tally, margins, *rec)
    return SimpleNamespace(P=P, S=S, B=B, work=work, scale=sc, marks=marks, tally=tally, margins=margins, marks_order_free=same, nngb=nngb)


def _accretion_post(P, B, k, prm, work, sc, tally, margins, i, b, enc, fws, sfws, sment, ssment, gv, sgv, mgas):
    """blackhole_accretion_reduce (PRIMARY) and blackhole_accretion_postprocess, :373-468, with the scales carried along"""
    f64 = np.float64
    B["encounter"][b] = enc
    work["BH_FeedbackWeightSum"][b], sc["work.BH_FeedbackWeightSum"][b] = f64(fws), f64(sfws)
    work["MgasEnc"][b], sc["work.MgasEnc"][b] = f64(mgas), f64(mgas)
    mass0, dens, atime = LD(B["Mass"][b]), LD(B["Density"][b]), LD(prm.atime)
    vel = P["Vel"][i].astype(LD)
    mdot, smdot = LD(0), LD(0)
    medd = LD(prm.EddingtonConst) * mass0 * LD(prm.UnitTime_in_s) / LD(prm.HubbleParam)
    ent, sent = sment, ssment
    if dens > 0:
        tally["density_positive"] += 1
        ent, sent, gv, sgv = sment / dens, ssment / dens, gv / dens, sgv / dens
        dv, sdv = vel - gv, np.abs(vel) + sgv
        bh2, sbh2 = (dv * dv).sum() / (atime * atime), (2 * np.abs(dv) * sdv).sum() / (atime * atime)
        cs2 = GAMMA * ent * np.power(dens, GAMMA_MINUS1) * np.power(atime, -3 * GAMMA_MINUS1)
        scs2 = GAMMA * sent * np.power(dens, GAMMA_MINUS1) * np.power(atime, -3 * GAMMA_MINUS1)
        A, sA = cs2 + bh2, scs2 + sbh2
        norm = np.power(A, LD(1.5))
        if norm > 0:
            tally["norm_positive"] += 1
            mdot = 4 * PI * LD(prm.BlackHoleAccretionFactor) * LD(prm.GravInternal) * LD(prm.GravInternal) * mass0 * mass0 * (dens * LD(prm.a3inv)) / norm
            smdot = mdot * (1 + LD(1.5) * sA / A)
        else:
            tally["norm_zero"] += 1
    else:
        tally["density_zero"] += 1
    work["BH_Entropy"][b], sc["work.BH_Entropy"][b] = f64(ent), f64(sent)
    work["BH_SurroundingGasVel"][b], sc["work.BH_SurroundingGasVel"][b] = gv.astype(f64), sgv.astype(f64)
    eddf = LD(prm.BlackHoleEddingtonFactor)
    if eddf > 0:
        cap = eddf * medd
        _note(margins, "eddington", _dist(mdot, cap, smdot, cap))
        if mdot > cap:
            mdot, smdot = cap, cap
            tally["edd_capped"] += 1
        else:
            tally["edd_free"] += 1
    else:
        tally["edd_off"] += 1
    B["Mdot"][b], sc["B.Mdot"][b] = f64(mdot), f64(smdot)
    dtime = LD(k.dloga[int(P["TimeBinHydro"][i])]) / LD(prm.hubble)
    mass, smass = mass0 + mdot * dtime, abs(mass0) + smdot * dtime
    B["Mass"][b], sc["B.Mass"][b] = f64(mass), f64(smass)
    drag, sdrag = np.zeros(3, dtype=LD), np.zeros(3, dtype=LD)
    if prm.BH_DRAG > 0:
        fac, sfac = LD(0), LD(0)
        if prm.BH_DRAG == 1:
            fac, sfac = mdot / LD(P["Mass"][i]) * atime, smdot / LD(P["Mass"][i]) * atime
        if prm.BH_DRAG == 2:
            fac = eddf * medd / mass * atime
            sfac = fac * (1 + smass / mass)
        dv, sdv = vel - gv, np.abs(vel) + sgv
        drag, sdrag = -dv * fac, sdv * abs(fac) + np.abs(dv) * sfac
        tally["drag1" if prm.BH_DRAG == 1 else "drag2"] += 1
    else:
        tally["drag0"] += 1
    B["DragAccel"][b], sc["B.DragAccel"][b] = drag.astype(f64), sdrag.astype(f64)
    work["KEflag"][b] = 0
    kfe, skfe = LD(B["KineticFdbkEnergy"][b]), LD(0)
    if prm.BlackHoleKineticOn == 1:
        flag = 0
        edd, sedd = mdot / medd, smdot / medd
        lam = LD(prm.BHKE_EddingtonThrFactor)
        x = LD(prm.BHKE_EddingtonMFactor) * np.power(mass / LD(prm.BHKE_EddingtonMPivot), LD(prm.BHKE_EddingtonMIndex))
        _note(margins, "lam_x", _dist(lam, x, lam, x * (1 + abs(LD(prm.BHKE_EddingtonMIndex)) * smass / mass)))
        if lam > x:
            lam = x
            tally["ke_low_x"] += 1
        else:
            tally["ke_low_thr"] += 1
        _note(margins, "edd_ratio", _dist(edd, lam, sedd, lam))
        if edd < lam:
            flag = 1
            tally["ke_accumulate"] += 1
            rho_crit_baryon = LD(prm.OmegaBaryon) * 3 * (LD(prm.Hubble) * LD(prm.Hubble)) / (8 * PI * LD(prm.GravInternal))
            eps = (dens / (LD(prm.BHKE_SfrCritOverDensity) * rho_crit_baryon)) / LD(prm.BHKE_EffRhoFactor)
            _note(margins, "epsilon", _dist(eps, LD(prm.BHKE_EffCap), eps, LD(prm.BHKE_EffCap)))
            if eps > prm.BHKE_EffCap:
                eps = LD(prm.BHKE_EffCap)
                tally["eps_capped"] += 1
            else:
                tally["eps_free"] += 1
            c2 = LD(prm.LightOverUnitVel) * LD(prm.LightOverUnitVel)
            skfe = abs(kfe) + eps * (smdot * dtime * c2)
            kfe = kfe + eps * (mdot * dtime * c2)
        else:
            tally["ke_high"] += 1
        vd = LD(B["VDisp"][b])
        thr = LD(0.5) * vd * vd * mgas * LD(prm.BHKE_InjEnergyThr)
        if vd > 0:
            _note(margins, "ke_thresh", _dist(kfe, thr, max(skfe, abs(kfe)), thr))
        if vd > 0 and kfe > thr:
            flag = 2
            tally["ke_release"] += 1
        else:
            tally["vdisp_zero" if (not vd > 0 and kfe > thr) else "ke_hold"] += 1
        work["KEflag"][b] = flag
        B["KineticFdbkEnergy"][b], sc["B.KineticFdbkEnergy"][b] = f64(kfe), f64(skfe)
    else:
        tally["ke_off"] += 1


def feedback(acc, ids, queue, kf, prm, maxpart, rnd, eeqos, in_tree):
    """treewalk_run(tw_feedback) with haswork and the postprocess, on copies of what accretion() returned.  Returns a namespace: P, S,
    B, work, scale, effects [(row, queue position, kind, value, scale of the value)], counts (gas swallowed, holes swallowed),
    tally, margins."""
    P, S, B, work = acc.P.copy(), acc.S.copy(), acc.B.copy(), {k: v.copy() for k, v in acc.work.items()}
    sca = acc.scale
    ids = np.asarray(ids, dtype=np.uint64)
    k, kt, n = kicks(kf), prm.DensityKernelType, len(P)
    Z = _Set(P, S, ids, prm, in_tree)
    tally, margins, effects = dict.fromkeys(BRANCHES, 0), {}, []
    sc = _scales(P, S, B, work)
    for name in ("B.Mdot", "B.DragAccel", "work.BH_FeedbackWeightSum", "work.BH_Entropy", "work.BH_SurroundingGasVel", "work.MgasEnc"):
        sc[name] = sca[name].copy()
    seed = LD(prm.SeedBHDynMass)
    gas_rows = Z.cand[Z.isgas]
    vp_gas, vps_gas = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    if len(gas_rows):
        vp_gas[gas_rows], vps_gas[gas_rows] = velpred(P, S, k, gas_rows, True)
    hole_rows = Z.cand[Z.ishole]
    vp_bh, vps_bh = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    if len(hole_rows):
        vp_bh[hole_rows], vps_bh[hole_rows] = velpred(P, S, k, hole_rows, False)
    sphmark = np.zeros(len(Z.cand), dtype=np.uint64)
    sphmark[Z.isgas] = work["SPH_SwallowID"][Z.cpi[Z.isgas]]
    bhmark = np.zeros(len(Z.cand), dtype=np.uint64)
    bhmark[Z.ishole] = work["BH_SwallowID"][Z.cpi[Z.ishole]]
    nrnd = np.uint64(len(rnd))
    rnd = np.asarray(rnd, dtype=np.float64)
    heat, heats, heat1 = np.zeros(len(S), dtype=LD), np.zeros(len(S), dtype=LD), np.zeros(len(S), dtype=LD)     # sum, scale, largest single
    nheat = np.zeros(len(S), dtype=np.int64)
    kick, kicks_ = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    nsph = nbh = 0
    post = []
    for t, i in enumerate(queue):
        i = int(i)
        b = int(P["PI"][i])
        if work["BH_SwallowID"][b] != 0:                                   # blackhole_feedback_haswork, :878-883
            tally["fb_no_work"] += 1
            continue
        myid = ids[i]
        h = float(P["Hsml"][i])
        idens, imtrack = LD(B["Density"][b]), LD(B["Mtrack"][b])
        fws, sfws = LD(work["BH_FeedbackWeightSum"][b]), LD(sca["work.BH_FeedbackWeightSum"][b])
        dtime = LD(k.dloga[int(P["TimeBinHydro"][i])]) / LD(prm.hubble)
        c2 = LD(prm.LightOverUnitVel) * LD(prm.LightOverUnitVel)
        fbe = LD(prm.BlackHoleFeedbackFactor) * LD(0.1) * LD(B["Mdot"][b]) * dtime * c2
        rfbe = LD(sca["B.Mdot"][b]) / LD(B["Mdot"][b]) if B["Mdot"][b] > 0 else LD(0)
        channel, kefb, rkefb = 0, LD(0), LD(0)
        if prm.BlackHoleKineticOn == 1 and work["KEflag"][b] > 0:
            channel = 1
            if work["KEflag"][b] == 2:
                kefb = LD(B["KineticFdbkEnergy"][b])
                rkefb = max(LD(sca["B.KineticFdbkEnergy"][b]) / kefb, LD(1)) if kefb > 0 else LD(0)
        tally["channel_thermal" if channel == 0 else "channel_kinetic_release" if work["KEflag"][b] == 2 else "channel_kinetic_hold"] += 1
        d, r2, acc_ = Z.around(i, margins)
        me = acc_ & (Z.cid == myid)
        dec = acc_ & ~me & Z.delayed
        rest = acc_ & ~me & ~dec
        tally["fb_self"] += int(me.sum())
        tally["fb_wind_decoupled"] += int(dec.sum())
        accm, saccm, accbh, saccbh, mom, smom, cprog = LD(0), LD(0), LD(0), LD(0), np.zeros(3, dtype=LD), np.zeros(3, dtype=LD), 0
        for j in np.flatnonzero(rest & Z.ishole):
            if bhmark[j] == 0:
                tally["bh_unmarked"] += 1
                continue
            if bhmark[j] != myid + np.uint64(1):
                tally["bh_marked_elsewhere"] += 1
                continue
            tally["bh_swallowed"] += 1
            o, ob = int(Z.cand[j]), int(Z.cpi[j])
            effects.append((o, t, 0, 0.0, 0.0))
            B["SwallowID"][ob] = int(bhmark[j]) - 1
            B["SwallowTime"][ob] = prm.atime
            P["Flags"][o] |= 2
            B["encounter"][ob] = 0
            nbh += 1
            cprog += int(B["CountProgs"][ob])
            accbh, saccbh = accbh + LD(B["Mass"][ob]), saccbh + LD(sca["B.Mass"][ob] if sca["B.Mass"][ob] > 0 else abs(B["Mass"][ob]))
            om = LD(Z.cmass[j])
            if seed > 0 and imtrack > 0:
                _note(margins, "seed", abs(float(LD(B["Mtrack"][ob]) / seed - 1)))
                if B["Mtrack"][ob] < prm.SeedBHDynMass:
                    om = LD(B["Mtrack"][ob])
                    tally["othermass_mtrack"] += 1
                else:
                    tally["othermass_particle"] += 1
            else:
                tally["othermass_imtrack_zero" if seed > 0 else "othermass_seed_off"] += 1
            accm, saccm = accm + om, saccm + abs(om)
            mom, smom = mom + om * vp_bh[o], smom + abs(om) * vps_bh[o]
        gas = np.flatnonzero(rest & Z.isgas)
        mk = sphmark[gas]
        inside = r2[gas] < h * h
        un = gas[(mk == 0) & inside]
        tally["gas_unmarked_inside"] += len(un)
        tally["gas_unmarked_outside"] += int(((mk == 0) & ~inside).sum())
        mintb = TIMEBINS
        if len(un):                                                       # `if(mintimebin > bin)` pair by pair, here in particle order
            bins = P["TimeBinHydro"][Z.cand[un]].astype(np.int64)
            before = np.minimum.accumulate(np.concatenate(([TIMEBINS], bins)))[:-1]
            tally["mintimebin_lowered"] += int((bins < before).sum())
            tally["mintimebin_kept"] += int((bins >= before).sum())
            mintb = int(bins.min())
        H = LD(h)
        dl = d[un].astype(LD)
        rl = np.sqrt((dl * dl).sum(axis=1))
        wk, wka = wk_values(kt, H, rl), wk_values(kt, H, rl, True)
        mj = Z.cmass[un].astype(LD)
        rows = Z.cand[un]
        if fws > 0 and fbe > 0 and channel == 0:
            ok = mj > 0
            tally["heat"] += int(ok.sum())
            tally["heat_zero_mass"] += int((~ok).sum())
            for o, m, w, wa in zip(rows[ok], mj[ok], wk[ok], wka[ok]):
                inj = fbe * m * w / fws
                val = inj / m
                sval = val * (1 + rfbe + sfws / fws + (wa / w if w > 0 else 0))
                effects.append((int(o), t, 2, float(val), float(sval)))
                s = int(P["PI"][o])
                heat[s], heats[s], heat1[s], nheat[s] = heat[s] + val, heats[s] + sval, max(heat1[s], val), nheat[s] + 1
                if eeqos is None:
                    tally["eeqos_absent"] += 1
                elif eeqos[o]:
                    P["Flags"][o] |= 8
                    tally["eeqos_flagged"] += 1
                else:
                    tally["eeqos_not"] += 1
        else:
            tally["heat_kinetic_channel" if channel != 0 else "heat_no_weight" if not fws > 0 else "heat_no_energy"] += len(un)
        if kefb > 0 and channel == 1 and idens > 0:
            tally["kick"] += len(un)
            for o, w, wa in zip(rows, wk, wka):
                dvel = np.sqrt(2 * kefb * w / idens)
                sdvel = dvel * (1 + LD(0.5) * (rkefb + (wa / w if w > 0 else 0)))
                effects.append((int(o), t, 3, float(dvel), float(sdvel)))
                theta = np.arccos(2 * LD(rnd[int((ids[o] + np.uint64(3)) % nrnd)]) - 1)
                phi = 2 * PI * LD(rnd[int((ids[o] + np.uint64(4)) % nrnd)])
                direc = np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], dtype=LD)
                kick[o], kicks_[o] = kick[o] + dvel * direc, kicks_[o] + sdvel * np.abs(direc)
        else:
            tally["kick_thermal_channel" if channel == 0 else "kick_nothing_released" if not kefb > 0 else "kick_no_density"] += len(un)
        tally["gas_marked_elsewhere"] += int(((mk != 0) & (mk != myid + np.uint64(1))).sum())
        for j in gas[mk == myid + np.uint64(1)]:
            o, s = int(Z.cand[j]), int(Z.cpi[j])
            tally["gas_swallowed"] += 1
            effects.append((o, t, 1, 0.0, 0.0))
            m = LD(Z.cmass[j])
            accm, saccm = accm + m, saccm + abs(m)
            mom, smom = mom + m * vp_gas[o], smom + abs(m) * vps_gas[o]
            P["Flags"][o] |= 1                                            # slots_mark_garbage
            S["ReverseLink"][s] = maxpart + 100
            nsph += 1
        post.append((i, b, accm, saccm, accbh, saccbh, mom, smom, cprog, mintb))
    # ---- the neighbours' side: heat with its cap, kicks
    f64 = np.float64
    for s in np.flatnonzero(nheat):
        enttou = np.power(LD(S["Density"][s]) * LD(prm.a3inv), GAMMA_MINUS1) / GAMMA_MINUS1
        u0 = LD(S["Entropy"][s]) * enttou
        cap = LD(prm.MaxThermalU)
        _note(margins, "max_u", _dist(u0 + heat[s], cap, abs(u0) + heats[s], cap))
        if u0 + heat[s] > cap:
            unew, su = cap, cap
            tally["heat_capped"] += 1
            tally["heat_capped_by_one" if u0 + heat1[s] > cap else "heat_capped_by_sum"] += 1
        else:
            unew, su = u0 + heat[s], abs(u0) + heats[s]
            tally["heat_free"] += 1
        S["Entropy"][s], sc["S.Entropy"][s] = f64(unew / enttou), f64(su / enttou)
    kicked = np.flatnonzero(np.any(kicks_ > 0, axis=1))
    if len(kicked):
        v0 = P["Vel"][kicked].astype(LD)
        P["Vel"][kicked], sc["P.Vel"][kicked] = (v0 + kick[kicked]).astype(f64), (np.abs(v0) + kicks_[kicked]).astype(f64)
    # ---- blackhole_feedback_reduce (PRIMARY) and blackhole_feedback_postprocess, :929-965
    for i, b, accm, saccm, accbh, saccbh, mom, smom, cprog, mintb in post:
        work["BH_accreted_Mass"][b], sc["work.BH_accreted_Mass"][b] = f64(accm), f64(saccm)
        work["BH_accreted_BHMass"][b], sc["work.BH_accreted_BHMass"][b] = f64(accbh), f64(saccbh)
        work["BH_accreted_momentum"][b], sc["work.BH_accreted_momentum"][b] = mom.astype(f64), smom.astype(f64)
        B["minTimeBin"][b] = mintb
        B["CountProgs"][b] += cprog
        sc["B.Mass"][b] = sca["B.Mass"][b]
        if accbh > 0:
            B["Mass"][b], sc["B.Mass"][b] = f64(LD(B["Mass"][b]) + accbh), f64(LD(sca["B.Mass"][b]) + saccbh)
            tally["bhmass_grows"] += 1
            tally["bhmass_only"] += int(not accm > 0)
        else:
            tally["bhmass_kept"] += 1
        if accm > 0:
            pm = LD(P["Mass"][i])
            v0 = P["Vel"][i].astype(LD)
            P["Vel"][i], sc["P.Vel"][i] = ((v0 * pm + mom) / (pm + accm)).astype(f64), ((np.abs(v0) * pm + smom) / (pm + accm)).astype(f64)
            mt = LD(B["Mtrack"][b])
            if seed > 0:
                _note(margins, "seed_sum", abs(float((mt + accm) / seed - 1)))
                _note(margins, "seed", abs(float(mt / seed - 1)))
            if seed > 0 and mt + accm < seed:
                B["Mtrack"][b], sc["B.Mtrack"][b] = f64(mt + accm), f64(abs(mt) + saccm)
                tally["mtrack_grows"] += 1
            elif mt < seed:
                sc["P.Mass"][i] = f64(mt + accm)                               # the float mass: compare() takes the float next to this value
                P["Mass"][i] = np.float32(mt + accm)
                B["Mtrack"][b] = prm.SeedBHDynMass
                tally["mtrack_saturates"] += 1
            else:
                sc["P.Mass"][i] = f64(pm + accm)
                P["Mass"][i] = np.float32(pm + accm)
                tally["mass_grows"] += 1
        else:
            tally["mass_nothing"] += 1
        if work["KEflag"][b] == 2:
            B["KineticFdbkEnergy"][b] = 0
            tally["ke_reset"] += 1
        else:
            sc["B.KineticFdbkEnergy"][b] = sca["B.KineticFdbkEnergy"][b]
            tally["ke_kept"] += 1
    # the scales of what the accretion walk left on holes this walk did not visit stay as they were
    done = np.zeros(len(B), dtype=bool)
    done[np.array([p[1] for p in post], dtype=np.int64)] = True
    for name in ("B.Mass", "B.KineticFdbkEnergy"):
        sc[name][~done] = sca[name][~done]
    return SimpleNamespace(P=P, S=S, B=B, work=work, scale=sc, effects=effects, counts=(nsph, nbh), tally=tally, margins=margins)
