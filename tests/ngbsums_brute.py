"""All-pairs restatements of the four neighbour-sum operators of csrc/sph_ngbsums.hip: stellar_density (stellar_density2.cpp),
wind_veldisp and bh_veldisp (veldisp2.cpp), bh_dynfric (bhdynfric.cpp).  No tree, no oracle, plain numpy, in the manner of
density_brute.py, whose kernel polynomials are reused.

Conventions, the same for every operator:
  - candidates are ALL particles whose type NOW lies in the wanted mask and that are not garbage (Flags & 1): what a walk over a tree
    built before some particles changed type or were marked garbage has to deliver, since such particles are passed over;
  - the separation is the minimum-image displacement `d - Box * round(d / Box)` in f64, and the distance test is taken on
    r2 = d0^2 + d1^2 + d2^2 in f64 over all candidates;
  - a pair exactly Box / 2 apart in a coordinate (a lattice of an even number of cells has them) is the same distance under
    either image, and round-half-even, rint and the strict comparisons of the reference all keep the plain difference, so the sign
    of the Hubble term of such a pair is the same everywhere too; above Box / 2 the minimum image gives every particle once;
  - pair terms are formed and accumulated in np.longdouble (only for the candidates inside the largest radius of the pass) and
    rounded to f64 once; the decisions (the running cut, ngb_narrow_down, the done rules, the exits) are taken in f64 on those sums;
  - every signed sum comes with the sum of the absolute values of its terms (`abs_*`), the scale its rounding error goes with;
  - every decision whose outcome jumps records its margin in `margins` (smallest over targets and passes): the relative distance of
    the nearest candidate from any trial or kernel radius ("radius"), of a kernel-weighted count from DesNumNgb and from the integer
    ngb_narrow_down compares with ("count"), of the chosen count from the band edges ("band"), of the gap between the two nearest
    counts ("close"), of R - L from the collapse limit ("collapse"), of R from 0.99 Box ("open"), and of the two lowest
    potentials from each other ("potential").  The clamps `hs > R`, `hs < L` and the 4 hs cap are min / max of continuous values
    and need none; the neighbour counts of the wind loop are integers and are compared exactly.

The running cut of the reference (`maxcmpte`: once the sum of radius k exceeds DesNumNgb, radii above k are no longer added to)
depends on the order of the walk only in WHICH radii stop being added to and when: the terms are non-negative, so a radius is cut
only after a smaller one has exceeded DesNumNgb for good, and the final maxcmpte is 1 + the first index whose COMPLETE sum exceeds
DesNumNgb.  The sums of every radius below the final maxcmpte are complete, and nothing else is read afterwards: computed that way.
"""
import numpy as np

import density_brute as db
from density_brute import LD, KERNELS, min_image

ST_NHSML = 10                # NHSML, stellar_density2.cpp
WV_NH = 5                    # NWINDHSML, veldisp2.cpp
WV_NUMDMNGB = 40
WV_MAXDEV = 1
MAXITER = 400                # treewalk2.h:21
BHPOTVALUEINIT = 1.0e29

ND_BRANCHES = ("closed", "open_extrap", "open_cap", "open_noslope", "clamp_R", "L0_first", "L0_slope", "L0_noslope", "clamp_L")
STELLAR_BRANCHES = ND_BRANCHES + ("band", "collapse", "redo")
WIND_BRANCHES = ND_BRANCHES + ("band", "collapse", "collapse_box", "redo", "vd_positive", "vd_not_positive")
BHVD_BRANCHES = ("written", "no_dm", "vd_not_positive")
DYNFRIC_BRANCHES = ("minpot_lowered", "minpot_kept", "dens_positive", "dens_zero")


def _pow3(x):
    return np.power(x, 3.0)


def _cbrt(x):
    return np.power(x, 1.0 / 3)          # pow(x, 1. / 3) as the reference writes it: NaN below zero


def _note(margins, name, values):
    values = np.asarray(values, dtype=np.float64)
    if values.size:
        margins[name] = min(margins.get(name, np.inf), float(np.min(values)))


def velpred(vel, treeacc, gravpm, bin_grav, gravkicks, FgravkickB):
    """DM_VelPred, density2.h:104-111: (Vel + gravkicks[bin] * FullTreeGravAccel) + GravPM * FgravkickB in f64, no contraction"""
    gk = np.asarray(gravkicks, dtype=np.float64)[np.asarray(bin_grav, dtype=np.int64)]
    return (np.asarray(vel, dtype=np.float64) + gk[:, None] * np.asarray(treeacc, dtype=np.float64)) + \
        np.asarray(gravpm, dtype=np.float64) * float(FgravkickB)


def wk_values(ktype, H, r, absolute=False):
    """the kernel at distance r for support radius H, in the precision of the arguments"""
    support, sigma = KERNELS[ktype]
    half = support / 2.0
    return sigma * (half / H) ** 3 * db.wk_int(ktype, r / H * half, absolute)


class Pairs:
    """f64 squared minimum-image distances of `targets` to `cands` (all pairs), and per target the sorted distances"""

    def __init__(self, pos, targets, cands, box, chunk=128):
        self.pos, self.targets, self.cands, self.box = pos, np.asarray(targets, dtype=np.int64), np.asarray(cands, dtype=np.int64), box
        nt, nc = len(self.targets), len(self.cands)
        self.r2 = np.empty((nt, nc))
        for k in range(0, nt, chunk):
            d = min_image(pos[self.targets[k:k + chunk]][:, None, :] - pos[self.cands][None, :, :], box)
            self.r2[k:k + chunk] = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        self.rs = np.sort(np.sqrt(self.r2), axis=1)

    def select(self, rows, rmax2, nonzero=False):
        """pairs (position in rows, candidate position) with r2 < rmax2[row], grouped by row; LD displacement; f64 r2"""
        sub = self.r2[rows]
        m = sub < rmax2[:, None]
        if nonzero:
            m &= sub > 0
        ti, gj = np.nonzero(m)
        d = min_image(self.pos[self.targets[rows[ti]]] - self.pos[self.cands[gj]], self.box)
        counts = np.bincount(ti, minlength=len(rows))
        starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
        return ti, gj, d.astype(LD), sub[ti, gj], starts, counts == 0, counts

    def radius_margin(self, rows, radii):
        """min over rows and radii of |r / radius - 1| for the candidate nearest to each radius (r = 0 pairs left out: `r > 0` is
        an exact test)"""
        radii = np.asarray(radii, dtype=np.float64).reshape(len(rows), -1)
        nc = self.rs.shape[1]
        if nc == 0 or len(rows) == 0:
            return np.inf
        best = np.inf
        for a, i in enumerate(rows):
            row = self.rs[i]
            k = np.searchsorted(row, radii[a])
            near = np.concatenate([row[np.clip(k - 1, 0, nc - 1)], row[np.clip(k, 0, nc - 1)]])
            rr = np.concatenate([radii[a], radii[a]])
            ok = near > 0
            if ok.any():
                best = min(best, float(np.abs(near[ok] / rr[ok] - 1).min()))
        return best


def _seg(x, starts, empty):
    """sums of consecutive segments of x in long double, rounded to f64 once; zero for empty segments (targets with no neighbour,
    which may come last: the starts of the non-empty segments alone delimit them)"""
    out = np.zeros(len(starts), dtype=LD)
    full = ~empty
    if full.any():
        out[full] = np.add.reduceat(np.asarray(x, dtype=LD), starts[full])
    return out.astype(np.float64)


def trial_radii(nh, left, right, h, box, stellar):
    """stellareffhsml (stellar_density2.cpp:38-54) / vdispeffdmradius (veldisp2.cpp:216-229): nh radii evenly spaced in volume"""
    left, right = left.copy(), right.copy()
    opn = right > 0.99 * box
    right[opn] = (h * ((1. + nh) / nh) if stellar else h)[opn]
    z = left == 0
    left[z] = 0.1 * h[z]
    rvol, lvol = _pow3(right), _pow3(left)
    k = np.arange(nh, dtype=np.float64)
    return _cbrt((1. * k[None, :] + 1) / (1. * nh + 1) * (rvol - lvol)[:, None] + lvol[:, None])


def narrow_down(R, L, radius, num, maxcmpt, desi, box, tally, margins, float_counts):
    """ngb_narrow_down, treewalk.c:1349-1406, for a whole queue.  Updates R and L in place; returns (new radius, close index)."""
    nt, nh = radius.shape
    rows = np.arange(nt)
    with np.errstate(all="ignore"):
        valid = np.arange(nh)[None, :] < maxcmpt[:, None]
        dist = np.where(valid, np.abs(num - desi), np.inf)
        close = np.argmin(dist, axis=1)                       # the first of equal distances, as the strict `<` of the reference
        if float_counts:
            _note(margins, "count", np.abs(num - desi)[valid])
            if nh > 1:
                two = np.sort(dist, axis=1)[:, :2]
                # equal distances of equal counts (all zero below the first neighbour) are the same bits: the first is kept exactly
                gap = two[:, 1] - two[:, 0]
                _note(margins, "close", gap[np.isfinite(two[:, 1]) & (gap > 0)])
        stop = np.zeros(nt, dtype=bool)
        for j in range(nh):
            act = valid[:, j] & ~stop
            lo = act & (num[:, j] < desi)
            L[lo] = radius[lo, j]
            hi = act & (num[:, j] > desi)
            R[hi] = radius[hi, j]
            stop |= hi
        hs = radius[rows, close].copy()
        m1, m2 = maxcmpt - 1, np.maximum(maxcmpt - 2, 0)
        rl, rl1, nl, nl1 = radius[rows, m1], radius[rows, m2], num[rows, m1], num[rows, m2]
        opn = R > 0.99 * box
        _note(margins, "open", np.abs(R / (0.99 * box) - 1))
        sl = opn & (maxcmpt > 1) & (rl > rl1)
        dn = np.where(sl, (nl - nl1) / np.where(sl, _pow3(rl) - _pow3(rl1), 1.0), 0.0)
        newh = 4 * hs
        ex = opn & (dn > 0)
        cand = _cbrt(_pow3(hs) + (desi - nl) / np.where(ex, dn, 1.0))
        use = ex & (cand < newh)
        hs = np.where(opn, np.where(use, cand, newh), hs)
        over = hs > R
        hs = np.where(over, R, hs)
        z = L == 0
        dn0 = np.where(radius[:, 1] > radius[:, 0], (num[:, 1] - num[:, 0]) / (_pow3(radius[:, 1]) - _pow3(radius[:, 0])), 0.0)
        first = z & (maxcmpt == 1) & (radius[:, 0] > 0)
        dn0 = np.where(first, num[:, 0] / _pow3(radius[:, 0]), dn0)
        go = z & (dn0 > 0)
        hs = np.where(go, _cbrt(_pow3(hs) + (desi - num[:, 0]) / np.where(go, dn0, 1.0)), hs)
        under = hs < L
        hs = np.where(under, L, hs)
    for name, m in (("closed", ~opn), ("open_extrap", use), ("open_cap", ex & ~use), ("open_noslope", opn & ~ex), ("clamp_R", over),
                    ("L0_first", go & first), ("L0_slope", go & ~first), ("L0_noslope", z & ~go), ("clamp_L", under)):
        tally[name] += int(m.sum())
    return hs, close


def stellar_density(pos, ptype, flags, mass, density, hsml, queue, box, ktype, DesNumNgb, MaxNgbDeviation, SPHWeighting):
    """stellar_density(): the whole loop for the stars `queue` (particle indices) over the gas.  `density`: by particle (read for gas).
    Returns a dict with Hsml, StarVolumeSPH, NumNgb (by queue position), niterations (the passes the longest star needs),
    hsml_max_tried (the largest radius any pass searched with or left), tally, margins, npairs_first."""
    pos = np.asarray(pos, dtype=np.float64)
    queue = np.asarray(queue, dtype=np.int64)
    cands = np.flatnonzero((np.asarray(ptype) == 0) & ((np.asarray(flags) & 1) == 0))
    P = Pairs(pos, queue, cands, box)
    nq = len(queue)
    hs = np.asarray(hsml, dtype=np.float64)[queue].copy()
    L, R = np.zeros(nq), np.full(nq, float(box))
    vol, ngb = np.full(nq, np.nan), np.full(nq, np.nan)
    volj = np.asarray(mass, dtype=np.float64).astype(LD) / np.asarray(density, dtype=np.float64).astype(LD)
    desi = int(DesNumNgb)
    tally, margins = dict.fromkeys(STELLAR_BRANCHES, 0), {}
    act = np.arange(nq)
    niter, tried, npairs_first = 0, 0.0, np.zeros(0, dtype=np.int64)
    fourpi3 = LD(4) * np.pi / 3
    while len(act):
        he = trial_radii(ST_NHSML, L[act], R[act], hs[act], box, True)
        he2 = he * he
        tried = max(tried, float(he[:, -1].max()))
        _note(margins, "radius", P.radius_margin(act, he))
        ti, gj, dl, r2, starts, empty, counts = P.select(act, he2[:, -1])
        if niter == 0:
            npairs_first = counts
        r = np.sqrt((dl * dl).sum(axis=1))
        vj = volj[cands[gj]]
        Ngb, Vol = np.zeros((len(act), ST_NHSML)), np.zeros((len(act), ST_NHSML))
        for k in range(ST_NHSML):
            inside = r2 < he2[ti, k]
            H = he[ti, k].astype(LD)
            wk = np.where(inside, wk_values(ktype, H, r), 0)
            Ngb[:, k] = _seg(wk * (fourpi3 * H * H * H), starts, empty)
            Vol[:, k] = _seg(vj * wk if SPHWeighting else np.where(inside, vj, 0), starts, empty)
        exceeds = Ngb > DesNumNgb
        maxcmpt = np.where(exceeds.any(axis=1), np.argmax(exceeds, axis=1) + 1, ST_NHSML)
        valid = np.arange(ST_NHSML)[None, :] < maxcmpt[:, None]
        _note(margins, "count", np.abs(Ngb - DesNumNgb)[valid])
        La, Ra = L[act], R[act]
        hnew, close = narrow_down(Ra, La, he, Ngb, maxcmpt, desi, box, tally, margins, True)
        rows = np.arange(len(act))
        nc = Ngb[rows, close]
        L[act], R[act], hs[act], ngb[act], vol[act] = La, Ra, hnew, nc, Vol[rows, close]
        tried = max(tried, float(hnew.max()))
        _note(margins, "band", np.minimum(np.abs(nc - (DesNumNgb - MaxNgbDeviation)), np.abs(nc - (DesNumNgb + MaxNgbDeviation))))
        out = (nc < DesNumNgb - MaxNgbDeviation) | (nc > DesNumNgb + MaxNgbDeviation)
        with np.errstate(all="ignore"):
            tight = (Ra - La) < 1.0e-4 * La
            _note(margins, "collapse", np.abs((Ra - La) / (1.0e-4 * La) - 1)[out & (La > 0)])
        tally["band"] += int((~out).sum())
        tally["collapse"] += int((out & tight).sum())
        tally["redo"] += int((out & ~tight).sum())
        act = act[out & ~tight]
        niter += 1
        assert niter <= MAXITER, "failed to converge the stellar density for %d stars" % len(act)
    return dict(Hsml=hs, StarVolumeSPH=vol, abs_StarVolumeSPH=np.abs(vol), NumNgb=ngb, Left=L, Right=R, niterations=niter,
                hsml_max_tried=tried, tally=tally, margins=margins, npairs_first=npairs_first)


def wind_veldisp(pos, ptype, flags, vel, vp, hsml, queue, box, Time, hubble):
    """winds_find_vel_disp, the dark-matter loop: for the gas particles `queue` over the DM (type 1).  `vp`: velpred() by particle.
    Returns a dict by queue position: VDisp (NaN where it is not written), DMRadius, NumDM, V1sum, V2sum, abs_V1sum of the chosen
    radius of the last pass, niterations, radius_max, tally, margins, npairs_first."""
    pos, vel, vp = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64), np.asarray(vp, dtype=np.float64)
    queue = np.asarray(queue, dtype=np.int64)
    cands = np.flatnonzero((np.asarray(ptype) == 1) & ((np.asarray(flags) & 1) == 0))
    P = Pairs(pos, queue, cands, box)
    nq = len(queue)
    dm = np.asarray(hsml, dtype=np.float64)[queue].copy()
    L, R = np.zeros(nq), np.full(nq, float(box))
    hub = LD(hubble * Time * Time)
    num, v1, v2, av1 = np.zeros(nq), np.zeros((nq, 3)), np.zeros(nq), np.zeros((nq, 3))
    vdisp = np.full(nq, np.nan)
    tally, margins = dict.fromkeys(WIND_BRANCHES, 0), {}
    act = np.arange(nq)
    niter, tried, npairs_first = 0, 0.0, np.zeros(0, dtype=np.int64)
    while len(act):
        rad = trial_radii(WV_NH, L[act], R[act], dm[act], box, False)
        tried = max(tried, float(rad[:, -1].max()))
        _note(margins, "radius", P.radius_margin(act, rad))
        ti, gj, dl, r2, starts, empty, counts = P.select(act, rad[:, -1] * rad[:, -1], nonzero=True)
        if niter == 0:
            npairs_first = counts
        r = np.sqrt(r2)                                              # f64, as the reference compares `r < rad[k]`
        t, j = queue[act][ti], cands[gj]
        e = (vp[j].astype(LD) - vel[t].astype(LD)) + hub * dl
        na = len(act)
        N, S1, S2, A1 = np.zeros((na, WV_NH)), np.zeros((na, WV_NH, 3)), np.zeros((na, WV_NH)), np.zeros((na, WV_NH, 3))
        for k in range(WV_NH):
            inside = r < rad[ti, k]
            N[:, k] = _seg(inside.astype(LD), starts, empty)
            for c in range(3):
                S1[:, k, c] = _seg(np.where(inside, e[:, c], 0), starts, empty)
                A1[:, k, c] = _seg(np.where(inside, np.abs(e[:, c]), 0), starts, empty)
            S2[:, k] = _seg(np.where(inside, (e * e).sum(axis=1), 0), starts, empty)
        exceeds = N > WV_NUMDMNGB
        maxcmpt = np.where(exceeds.any(axis=1), np.argmax(exceeds, axis=1) + 1, WV_NH)
        La, Ra = L[act], R[act]
        dnew, close = narrow_down(Ra, La, rad, N, maxcmpt, WV_NUMDMNGB, box, tally, margins, False)
        rows = np.arange(na)
        nc = N[rows, close]
        L[act], R[act], dm[act] = La, Ra, dnew
        num[act], v1[act], v2[act], av1[act] = nc, S1[rows, close], S2[rows, close], A1[rows, close]
        band = (nc >= WV_NUMDMNGB - WV_MAXDEV) & (nc <= WV_NUMDMNGB + WV_MAXDEV)
        with np.errstate(all="ignore"):
            tight = (Ra - La) < 5e-6 * La
            _note(margins, "collapse", np.abs((Ra - La) / (5e-6 * La) - 1)[~band & (La > 0)])
            done = band | tight
            s1, s2 = S1[rows, close], S2[rows, close]
            vd = s2 / nc
            for c in range(3):
                vd = vd - (s1[:, c] / nc) * (s1[:, c] / nc)
            wr = done & (vd > 0)
            vdisp[act[wr]] = np.sqrt(vd[wr] / 3)
        tally["band"] += int(band.sum())
        tally["collapse"] += int((~band & tight & (Ra < box)).sum())
        tally["collapse_box"] += int((~band & tight & (Ra == box)).sum())
        tally["redo"] += int((~done).sum())
        tally["vd_positive"] += int(wr.sum())
        tally["vd_not_positive"] += int((done & ~wr).sum())
        act = act[~done]
        niter += 1
        assert niter <= MAXITER, "failed to converge the wind velocity dispersion for %d particles" % len(act)
    return dict(VDisp=vdisp, DMRadius=dm, NumDM=num, V1sum=v1, V2sum=v2, abs_V1sum=av1, Left=L, Right=R, niterations=niter, radius_max=tried,
                tally=tally, margins=margins, npairs_first=npairs_first)


def bh_veldisp(pos, ptype, flags, vel, vp, hsml, queue, box):
    """blackhole_veldisp, veldisp2.cpp:20-199: count and moments of DM_VelPred - Vel_bh over the DM with 0 < r2 < Hsml^2.
    By queue position: NumDM, V1sumDM, V2sumDM, abs_V1sumDM, VDisp (NaN where it is not written)."""
    pos, vel, vp = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64), np.asarray(vp, dtype=np.float64)
    queue = np.asarray(queue, dtype=np.int64)
    cands = np.flatnonzero((np.asarray(ptype) == 1) & ((np.asarray(flags) & 1) == 0))
    P = Pairs(pos, queue, cands, box)
    h = np.asarray(hsml, dtype=np.float64)[queue]
    rows = np.arange(len(queue))
    tally, margins = dict.fromkeys(BHVD_BRANCHES, 0), {}
    _note(margins, "radius", P.radius_margin(rows, h))
    ti, gj, dl, r2, starts, empty, counts = P.select(rows, h * h, nonzero=True)
    e = vp[cands[gj]].astype(LD) - vel[queue[ti]].astype(LD)
    num = counts.astype(np.float64)
    v1 = np.stack([_seg(e[:, c], starts, empty) for c in range(3)], axis=1)
    av1 = np.stack([_seg(np.abs(e[:, c]), starts, empty) for c in range(3)], axis=1)
    v2 = _seg((e * e).sum(axis=1), starts, empty)
    vdisp = np.full(len(queue), np.nan)
    with np.errstate(all="ignore"):
        vd = v2 / num
        for c in range(3):
            vd = vd - np.power(v1[:, c] / num, 2)
        wr = (num > 0) & (vd > 0)
        vdisp[wr] = np.sqrt(vd[wr] / 3)
    tally["written"], tally["no_dm"], tally["vd_not_positive"] = int(wr.sum()), int((num == 0).sum()), int(((num > 0) & ~wr).sum())
    return dict(NumDM=num, V1sumDM=v1, abs_V1sumDM=av1, V2sumDM=v2, VDisp=vdisp, tally=tally, margins=margins, npairs_first=counts)


def bh_dynfric(pos, ptype, flags, mass, vel, vp, potential, hsml, queue, slots, box, ktype, method, typemask, MinPot, MinPotPos, MinPotVel):
    """blackhole_dynfric / blackhole_repos, bhdynfric.cpp:44-295, for the holes `queue` with BH slots `slots`: the candidate of
    lowest potential inside the kernel radius, reduced into copies of the caller's MinPot arrays (by slot), and for method > 0 the
    kernel-weighted mass, momentum and squared DM_VelPred of the stars (method 2: and of the DM) with their post-process.
    Returns MinPot, MinPotPos, MinPotVel, updated (by slot) and, by queue position, raw_minpot, dens, mom [nq, 3], v2, abs_mom,
    Density, Vel, RmsVel, plus tally and margins."""
    pos, vel, vp = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64), np.asarray(vp, dtype=np.float64)
    ptype, potential = np.asarray(ptype), np.asarray(potential, dtype=np.float64)
    queue, slots = np.asarray(queue, dtype=np.int64), np.asarray(slots, dtype=np.int64)
    cands = np.flatnonzero((((1 << ptype.astype(np.int64)) & typemask) != 0) & ((np.asarray(flags) & 1) == 0))
    P = Pairs(pos, queue, cands, box)
    h = np.asarray(hsml, dtype=np.float64)[queue]
    nq = len(queue)
    rows = np.arange(nq)
    tally, margins = dict.fromkeys(DYNFRIC_BRANCHES, 0), {}
    _note(margins, "radius", P.radius_margin(rows, h))
    ti, gj, dl, r2, starts, empty, counts = P.select(rows, h * h)
    j = cands[gj]
    raw = np.full(nq, BHPOTVALUEINIT)
    rpos, rvel = np.full((nq, 3), -1.0), np.zeros((nq, 3))
    for q in range(nq):
        jj = j[starts[q]:starts[q] + counts[q]]
        if len(jj) == 0:
            continue
        p = potential[jj]
        o = np.argsort(p, kind="stable")
        if p[o[0]] < raw[q]:
            raw[q], rpos[q], rvel[q] = p[o[0]], pos[jj[o[0]]], vel[jj[o[0]]]
        if len(jj) > 1:
            _note(margins, "potential", (p[o[1]] - p[o[0]]) / max(abs(p[o[0]]), abs(p[o[1]]), 1e-300))
    mp, mpp, mpv = np.array(MinPot, dtype=np.float64), np.array(MinPotPos, dtype=np.float64), np.array(MinPotVel, dtype=np.float64)
    upd = np.zeros(len(mp), dtype=np.int32)
    # the hole's own potential is a candidate: where it is the lowest the two values are the same bits, an exact comparison
    gap = np.abs(mp[slots] - raw) / np.maximum(np.maximum(np.abs(mp[slots]), np.abs(raw)), 1e-300)
    _note(margins, "potential", gap[mp[slots] != raw])
    better = mp[slots] > raw                      # BHReposResult::reduce, bhdynfric.cpp:106-118
    mp[slots[better]], mpp[slots[better]], mpv[slots[better]], upd[slots[better]] = raw[better], rpos[better], rvel[better], 1
    tally["minpot_lowered"], tally["minpot_kept"] = int(better.sum()), int((~better).sum())
    out = dict(MinPot=mp, MinPotPos=mpp, MinPotVel=mpv, updated=upd, raw_minpot=raw, tally=tally, margins=margins, npairs_first=counts)
    if method > 0:
        w = (ptype[j] == 4) | ((ptype[j] == 1) & (method > 1))
        H = h[ti].astype(LD)
        r = np.sqrt((dl * dl).sum(axis=1))
        mw = np.where(w, np.asarray(mass, dtype=np.float64)[j].astype(LD) * wk_values(ktype, H, r), 0)
        v = vp[j].astype(LD)
        dens = _seg(mw, starts, empty)
        mom = np.stack([_seg(mw * v[:, c], starts, empty) for c in range(3)], axis=1)
        amom = np.stack([_seg(mw * np.abs(v[:, c]), starts, empty) for c in range(3)], axis=1)
        v2 = _seg(mw * (v * v).sum(axis=1), starts, empty)
        pz = dens > 0                                  # BHDynFricOutput::postprocess, bhdynfric.cpp:66-82
        with np.errstate(all="ignore"):
            Vel = np.where(pz[:, None], mom / np.where(pz, dens, 1)[:, None], mom)
            Rms = np.where(pz, np.sqrt(v2 / np.where(pz, dens, 1)), v2)
        tally["dens_positive"], tally["dens_zero"] = int(pz.sum()), int((~pz).sum())
        out.update(dens=dens, mom=mom, abs_mom=amom, v2=v2, Density=dens, Vel=Vel, RmsVel=Rms)
    return out
