/* cooling_uvbg.hpp — get_local_UVBG (cooling_uvfluc.cpp:142-199) on the device, for the kernels that read per-particle arrays: cooling.hip's
 * and sfr.hip's.  A is the kernel's argument struct; it holds posm, ztab, znside, zbox, offset[3], mode, j21, zre, j21c[6], ss_grey, ss_fbar,
 * redshift and global, as CoolPartArgs does. */
#ifndef SHQ_COOLING_UVBG_HPP
#define SHQ_COOLING_UVBG_HPP
#include "common.hpp"

/* InterpNLinear<3>::eval_periodic (utils/interp.hpp:93-129) on the Zreion table: Min = 0, Max = BoxSize */
template <class A> __device__ inline double cool_zreion_at(const A &a, const double4 &p)
{
    const int ns = a.znside;
    const double step = (a.zbox - 0.0) / (ns - 1);
    const double x[3] = {p.x - a.offset[0], p.y - a.offset[1], p.z - a.offset[2]};
    long long xi[3];
    double f[3];
    for(int d = 0; d < 3; d++) {
        const double xd = (x[d] - 0.0) / step;
        const double fl = floor(xd);
        /* a position far outside the box (or not finite) still lands inside the table */
        xi[d] = (fl > -1e15 && fl < 1e15) ? (long long) fl : 0;
        f[d] = xd - (double) xi[d];
    }
    double ret = 0;
    for(int i = 0; i < 8; i++) {
        double filter = 1.0;
        long long l = 0;
        for(int d = 0; d < 3; d++) {
            const int foffset = (i & (1 << d)) ? 1 : 0;
            long long x1 = (xi[d] + foffset) % ns;
            if(x1 < 0)
                x1 += ns;
            filter *= foffset ? f[d] : (1 - f[d]);
            l = l * ns + x1;
        }
        ret += a.ztab[l] * filter;
    }
    return ret;
}
template <class A> __device__ inline void cool_local_uvbg(const A &a, long long i, CoolUV &uv)
{
    const CoolUV g = a.global;
    if(a.mode == SHQ_COOL_UVBG_J21) { /* get_local_UVBG_from_J21 (cooling_uvfluc.cpp:167-199) */
        const double J21 = a.j21[i];
        uv.zreion = a.zre[i];
        uv.gJH0 = a.j21c[0] * J21;
        uv.epsH0 = a.j21c[3] * J21 * 1.60218e-12;
        uv.gJHe0 = a.j21c[2] * J21;
        uv.epsHe0 = a.j21c[5] * J21 * 1.60218e-12;
        uv.gJHep = 0.;
        uv.epsHep = 0.;
        /* get_self_shield_dens (cooling_rates.cpp:226-235): the grey-opacity and fBar powers are the caller's */
        if(uv.gJH0 == 0)
            uv.self_shield_dens = 1e10;
        else {
            const double G12 = uv.gJH0 / 1e-12;
            uv.self_shield_dens = 6.73e-3 * a.ss_grey * pow(G12, 2. / 3) * a.ss_fbar;
        }
        return;
    }
    if(a.mode == SHQ_COOL_UVBG_GLOBAL) {
        uv = g;
        return;
    }
    /* get_local_UVBG_from_global (:142-165) */
    const double zreion = cool_zreion_at(a, a.posm[i]);
    if(zreion < a.redshift) {
        uv = CoolUV{0, 0, 0, 0, 0, 0, g.self_shield_dens, zreion};
        return;
    }
    uv = g;
    uv.zreion = zreion;
}

#endif
