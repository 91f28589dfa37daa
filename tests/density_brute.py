"""All-pairs restatement of density() with its Hsml loop: no tree, no oracle, plain numpy.

What the tree walk of the reference computes (LocalNgbTreeWalk::visit + DensityLocalTreeWalk::ngbiter, densitytree2.hpp:362-423)
is, per target, a sum over every gas particle whose minimum-image distance is below Hsml.  Here that sum is taken over ALL gas
particles with `d - Box * round(d / Box)`, so nothing of cull_node, of the node geometry or of the order of a walk enters: a
misreading of the cull that the oracle (oracle/sph.cpp) and the device kernels share shows up against this file.

Pair terms are formed in np.longdouble from the f64 minimum-image displacement and accumulated in np.longdouble, then rounded to
f64 once; the decisions of the Hsml update (density_check_neighbours, densitytree2.hpp:177-257) are taken in f64 on those rounded
sums, as the reference takes them.  The kernels are written from their piecewise polynomials (Price 2012; densitykernel.hpp).

Conventions that follow the reference where a "plain" sum could choose otherwise:
  - `r < Hsml` strict; a pair at r = 0 (the target itself when it is gas) adds to the wk sums and not to the gradient sums;
  - above Hsml = Box / 2 the minimum image still gives every particle ONCE (the reference walks nearest images only), so the
    sums stop growing like a sphere's: Hsml can run up to Right = Box, and the bracket collapses there with Hsml = Box exactly;
  - the postprocess runs after the update of every pass, so DhsmlEgyDensityFactor and DtHsml of the final pass carry the Hsml that
    pass leaves (it differs from the Hsml of the sums only where the pass ends on a floor or on the collapsed bracket).
"""
import numpy as np

GAMMA = 5.0 / 3.0
MAXITER = 400                                            # treewalk2.h:21
LD = np.longdouble

KERNELS = {1: (4, 1 / np.pi), 2: (6, 1 / (120 * np.pi)), 4: (5, 1 / (20 * np.pi))}     # type: (support 2H/h, sigma)
OUTCOMES = ("bracket_collapse", "bisect", "bisect_box", "grow_clamp", "shrink_clamp", "newton", "floor_R", "floor_band", "inband")


def _ipow(x, p):
    """x^p for a small integer p by multiplication (long double pow() is slow and no more exact)"""
    y = x
    for _ in range(p - 1):
        y = y * x
    return y


def wk_int(ktype, q, absolute=False):
    """the kernel's polynomial in q = r / h (h = 2H / support), zero from q = support / 2 on.  absolute: the sum of the absolute
    values of its terms instead (what rounding errors scale with where the terms cancel)"""
    q = np.asarray(q)
    z = np.zeros_like(q)
    c = lambda a, p: _ipow(np.where(q < a, a - q, z), p)             # noqa: E731  truncated power (a - q)_+^p
    s = 1 if absolute else -1
    if ktype == 1:
        return 0.25 * c(2, 3) + s * c(1, 3)
    if ktype == 2:
        return c(3, 5) + s * 6 * c(2, 5) + 15 * c(1, 5)
    if ktype == 4:
        return c(2.5, 4) + s * 5 * c(1.5, 4) + 10 * c(0.5, 4)
    raise ValueError(ktype)


def dwk_int(ktype, q, absolute=False):
    q = np.asarray(q)
    z = np.zeros_like(q)
    c = lambda a, p: _ipow(np.where(q < a, a - q, z), p)             # noqa: E731
    s = 1 if absolute else -1
    if ktype == 1:
        return s * 0.75 * c(2, 2) + 3 * c(1, 2)
    if ktype == 2:
        return s * 5 * c(3, 4) + 30 * c(2, 4) + s * 75 * c(1, 4)
    if ktype == 4:
        return s * 4 * c(2.5, 3) + 20 * c(1.5, 3) + s * 40 * c(0.5, 3)
    raise ValueError(ktype)


def kernel_values(ktype, H, u, absolute=False):
    """(wk, dwk, dW, volume) at u = r / H for support radius H, in the precision of the arguments.  absolute: wk, dwk and dW with
    every term taken by its absolute value (the scale of their rounding errors)"""
    support, sigma = KERNELS[ktype]
    H = np.asarray(H)
    half = support / 2.0
    wknorm = sigma * (half / H) ** 3
    q = u * half
    wk = wknorm * wk_int(ktype, q, absolute)
    dwk = wknorm * half / H * dwk_int(ktype, q, absolute)
    dW = (3 * wk / H + u * dwk) if absolute else -(3 * wk / H + u * dwk)
    return wk, dwk, dW, 4 * np.pi / 3 * H ** 3


def desnumngb(ktype, eta=1.0):
    return 4.0 / 3 * np.pi * (KERNELS[ktype][0] / 2.0 * eta) ** 3


def min_image(d, box):
    return d - box * np.round(d / box)


def _seg_sum(x, starts, empty):
    """sums of consecutive segments of x (long double), zero for empty segments"""
    if len(x) == 0:
        return np.zeros(len(starts), dtype=LD)
    s = np.add.reduceat(x, np.minimum(starts, len(x) - 1))
    s[empty] = 0
    return s


def pair_sums(pos, vel, evp, mass, gas, targets, hsml, box, ktype):
    """The sums of ngbiter for `targets` (particle indices) with radii `hsml` over the gas particles `gas` (indices).
    Returns a dict of f64 arrays [len(targets)] / [len(targets), 3]; `abs_*`: the sums of the absolute values of the terms."""
    nt = len(targets)
    d = min_image(pos[targets][:, None, :] - pos[gas][None, :, :], box)           # f64; exact for pairs closer than Box / 2
    r2 = (d * d).sum(axis=2)
    ti, gj = np.nonzero(r2 < (hsml * hsml)[:, None])                              # row-major: grouped by target
    counts = np.bincount(ti, minlength=nt)
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    empty = counts == 0
    dl = d[ti, gj].astype(LD)
    r = np.sqrt((dl * dl).sum(axis=1))
    H = hsml[ti].astype(LD)
    wk, dwk, dW, vol = kernel_values(ktype, H, r / H)
    j = gas[gj]
    mj = mass[j].astype(LD)
    ej = evp[j].astype(LD)
    S = lambda x: _seg_sum(x, starts, empty).astype(np.float64)                   # noqa: E731  rounded to f64 once
    out = dict(NumNgb=S(wk * vol), Rho=S(mj * wk), DhsmlDensity=S(mj * dW), EgyRho=S(mj * ej * wk), DhsmlEgyDensity=S(mj * ej * dW),
               abs_DhsmlDensity=S(np.abs(mj * dW)), abs_DhsmlEgyDensity=S(np.abs(mj * ej * dW)), npairs=counts)
    nz = r > 0
    fac = np.where(nz, mj * dwk / np.where(nz, r, 1), 0)
    dv = (vel[targets][ti] - vel[j]).astype(LD)
    divt = -fac * (dl * dv).sum(axis=1)
    rott = fac[:, None] * np.stack([dv[:, 1] * dl[:, 2] - dv[:, 2] * dl[:, 1], dv[:, 2] * dl[:, 0] - dv[:, 0] * dl[:, 2],
                                    dv[:, 0] * dl[:, 1] - dv[:, 1] * dl[:, 0]], axis=1)
    gradt = fac[:, None] * dl
    out["Div"], out["abs_Div"] = S(divt), S(np.abs(divt))
    out["Rot"] = np.stack([S(rott[:, k]) for k in range(3)], axis=1)
    out["abs_Rot"] = np.stack([S(np.abs(rott[:, k])) for k in range(3)], axis=1)
    out["GradRho"] = np.stack([S(gradt[:, k]) for k in range(3)], axis=1)
    out["abs_GradRho"] = np.stack([S(np.abs(gradt[:, k])) for k in range(3)], axis=1)
    return out


def check_neighbours(N, DensFac, hs, L, R, des, dev, box, minhsml, counters):
    """density_check_neighbours for a whole queue, decisions in f64.  Updates L and R in place; returns (new Hsml, done)."""
    with np.errstate(all="ignore"):
        out = (N < des - dev) | (N > des + dev)
        collapse = out & ((R - L) < 1.0e-5 * R)
        upd = out & ~collapse
        low = upd & (N < des)
        high = upd & ~low
        L[low] = hs[low]
        R[high] = hs[high]
        inner = (R < box) & (L > 0)
        bis = upd & (inner | (hs * 1.26 > 0.99 * box))
        fb = upd & ~bis
        fac = np.where(N > 0, 1 - (N - des) / (3 * np.where(N > 0, N, 1)) * DensFac, 1.26)
        grow = fb & (R > 0.99 * box) & (L > 0) & ((DensFac <= 0) | (np.abs(N - des) >= 0.5 * des) | (fac > 1.26))
        fac = np.where(grow, 1.26, fac)
        shrink = fb & (R < 0.99 * box) & (L == 0) & ((DensFac <= 0) | (fac < 1. / 3))
        fac = np.where(shrink, 1. / 3, fac)
        new = np.where(bis, np.cbrt(0.5 * (L ** 3 + R ** 3)), hs * fac)
        floor_R = upd & (R < minhsml)
        new = np.where(floor_R, minhsml, new)
        new = np.where(collapse, R, new)
        band = ~out
        floor_band = band & (hs < minhsml)
        new = np.where(band, np.where(floor_band, minhsml, hs), new)
        done = collapse | floor_R | band
    for name, m in (("bracket_collapse", collapse), ("bisect", bis & inner), ("bisect_box", bis & ~inner), ("grow_clamp", grow),
                    ("shrink_clamp", shrink), ("newton", fb & ~grow & ~shrink), ("floor_R", floor_R), ("floor_band", floor_band),
                    ("inband", band & ~floor_band)):
        counters[name] += int(m.sum())
    return new, done


def dhsml_density_factor(s, h):
    with np.errstate(all="ignore"):
        return 1 / (1 + s["DhsmlDensity"] * h / (3 * s["Rho"]))


def postprocess(s, evp, isgas, h_old, h_new):
    """DensityOutput::postprocess, densitytree2.hpp:117-175, on a pass's sums `s` (radii h_old) and the Hsml the update leaves;
    `abs_X`: X formed from the sums of the absolute values of its terms, the scale of the rounding error of X"""
    rho, DensFac = s["Rho"], dhsml_density_factor(s, h_old)
    with np.errstate(all="ignore"):
        f = {"Density": rho, "NumNgb": s["NumNgb"], "DhsmlDensityFactor": DensFac,
             "EgyWtDensity": np.where(isgas, s["EgyRho"] / np.where(isgas, evp, 1), np.nan),
             "DhsmlEgyDensityFactor": np.where(isgas, s["DhsmlEgyDensity"] * (h_new / (3 * s["EgyRho"])) * -DensFac, np.nan),
             "DivVel": s["Div"] / rho, "abs_DivVel": s["abs_Div"] / rho,
             "CurlVel": np.where(isgas, np.linalg.norm(s["Rot"], axis=1) / rho, np.nan),
             "abs_CurlVel": np.linalg.norm(s["abs_Rot"], axis=1) / rho,
             "GradRho_mag": np.where(isgas, np.linalg.norm(s["GradRho"], axis=1), np.nan),
             "abs_GradRho_mag": np.linalg.norm(s["abs_GradRho"], axis=1)}
        f["DtHsml"] = (1.0 / 3) * f["DivVel"] * h_new
        f["abs_DtHsml"] = (1.0 / 3) * f["abs_DivVel"] * h_new
    return f


def entvarpred(entropy):
    return np.exp(1.0 / GAMMA * np.log(entropy))                     # SPH_EntVarPred with zero kicks, density2.h:115-128


def single_pass(pos, ptype, mass, vel, entropy, hsml, box, ktype, targets, chunk=64):
    """the fields of ONE pass at fixed radii for `targets` (no update): dict of arrays [len(targets)].  For the scales of the signed
    sums where only a converged state is at hand."""
    pos, vel, mass = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    ptype, hsml, targets = np.asarray(ptype), np.asarray(hsml, dtype=np.float64), np.asarray(targets, dtype=np.int64)
    gas = np.flatnonzero(ptype == 0)
    evp = np.zeros(len(pos))
    evp[gas] = entvarpred(np.asarray(entropy, dtype=np.float64)[gas])
    parts = []
    for k in range(0, len(targets), chunk):
        q = targets[k:k + chunk]
        parts.append(postprocess(pair_sums(pos, vel, evp, mass, gas, q, hsml[q], box, ktype), evp[q], ptype[q] == 0, hsml[q], hsml[q]))
    if not parts:
        return {}
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def density(pos, ptype, mass, vel, entropy, hsml, box, ktype, DesNumNgb, DesNumNgbBH, MaxNumNgbDeviation, MinGasHsml, BlackHoleOn=0,
            active=None):
    """density() with update_hsml = 1, DoEgyDensity = 1 and zero kick factors, for the gas (type 0) and black-hole (type 5) particles
    of `active` (None: all).  `entropy`, and every returned field, is indexed by particle (BH rows of the gas-only fields are NaN).
    Returns a dict: Hsml (all particles), the fields, `abs_*` scales, niterations, counters, margin, npairs_first (the neighbours
    of each target of the first pass)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    ptype = np.asarray(ptype)
    mass = np.asarray(mass, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    gas = np.flatnonzero(ptype == 0)
    evp = np.zeros(n)
    evp[gas] = entvarpred(np.asarray(entropy, dtype=np.float64)[gas])
    # a pair at exactly Box / 2 in a coordinate has two nearest images; it is at least Box / 2 away, so the choice can only matter
    # to a radius above Box / 2 (asserted per pass; a lattice of an even number of cells has such pairs, far outside its radii)
    g = pos[gas]
    half_pairs = any(np.any(np.abs(pos[:, None, k] - g[None, :, k]) == 0.5 * box) for k in range(3))
    hs = np.array(hsml, dtype=np.float64)
    L, R = np.zeros(n), np.full(n, float(box))
    queue = np.arange(n) if active is None else np.asarray(active, dtype=np.int64)
    queue = queue[(ptype[queue] == 0) | (ptype[queue] == 5)]
    des_all = np.where((ptype == 5) & bool(BlackHoleOn), DesNumNgbBH, DesNumNgb)
    counters = dict.fromkeys(OUTCOMES, 0)
    names = ("Density", "EgyWtDensity", "DhsmlEgyDensityFactor", "DivVel", "CurlVel", "DtHsml", "GradRho_mag", "NumNgb",
             "abs_DivVel", "abs_CurlVel", "abs_GradRho_mag", "abs_DtHsml", "DhsmlDensityFactor")
    res = {k: np.full(n, np.nan) for k in names}
    margin, niter, npairs_first = np.inf, 0, np.zeros(0, dtype=np.int64)
    while True:
        q = queue
        s = pair_sums(pos, vel, evp, mass, gas, q, hs[q], box, ktype) if len(q) else None
        if len(q):
            assert not half_pairs or hs[q].max() <= 0.5 * box, "a pair at exactly Box / 2 within reach: the minimum image is ambiguous"
            N, rho, h_old = s["NumNgb"], s["Rho"], hs[q]
            if niter == 0:
                npairs_first = s["npairs"]
            DensFac = dhsml_density_factor(s, h_old)
            des = des_all[q]
            margin = min(margin, min(np.abs(N - t).min() for t in (des - MaxNumNgbDeviation, des, des + MaxNumNgbDeviation)))
            Lq, Rq = L[q], R[q]
            h_new, done = check_neighbours(N, DensFac, h_old, Lq, Rq, des, MaxNumNgbDeviation, box, MinGasHsml, counters)
            L[q], R[q], hs[q] = Lq, Rq, h_new
            f = postprocess(s, evp[q], ptype[q] == 0, h_old, h_new)
            for k, v in f.items():
                res[k][q] = v
            queue = q[~done]
        niter += 1
        if len(queue) == 0:
            break
        assert niter <= MAXITER, "failed to converge density for %d particles" % len(queue)
    res.update(Hsml=hs, niterations=niter, counters=counters, margin=float(margin), npairs_first=npairs_first)
    return res
