/* nulra_host_main.cpp — a stand-alone program for the host sanitizers (no python, no GPU): csrc/nulra_host.hip (the linear-response
 * neutrino engine of nulra_math.hpp driven in plain loops) with the one function it needs of the rest of the library, and a main that
 * runs first init, twelve steps under the 0.009 rule, the rebin branch, hybrid steps with the refined nodes, a state round trip (bit
 * equal) and the mode table.
 *
 *     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ishenqi_amd/csrc \
 *         tools/nulra_host_main.cpp -o nulra_host_check && ./nulra_host_check */
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "nulra_host.hip"

static char last_error[1024];
void shq_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

struct Cosmo {
    double H0, mnu[3], deg[3], OmegaNu1, nufrac, crit;
    int hybrid;
};
static const double kBtnu = 8.61734e-5 * 0.7137658555036082 * 1.00328 * 2.7255;
static double single0(const Cosmo *c, double a, int mi)
{
    const double m = c->mnu[mi];
    return m <= 0 ? 1.1e-5 / pow(a, 4) : m / 93.14 / 0.49 / pow(a, 3) * sqrt(1 + pow(3.15 * kBtnu / (a * m), 2));
}
static double partnu(const Cosmo *c, double a) { return c->hybrid && a > c->crit ? c->nufrac : 0; }
static double cb_hubble(double a, int, void *u)
{
    const Cosmo *c = (const Cosmo *) u;
    return c->H0 * sqrt(0.2793 / pow(a, 3) + (1 - 0.2793) + 5.04672e-5 / pow(a, 4));
}
static double cb_single(double a, int mi, void *u)
{
    const Cosmo *c = (const Cosmo *) u;
    return single0(c, a, mi) - single0(c, 1, mi) * partnu(c, a) / pow(a, 3);
}
static double cb_nopart(double a, int, void *u)
{
    const Cosmo *c = (const Cosmo *) u;
    double s = 0;
    for(int i = 0; i < 3; i++)
        s += c->deg[i] * single0(c, a, i);
    return s - c->OmegaNu1 * partnu(c, a) / pow(a, 3);
}

#define OK(call)                                                                    \
    do {                                                                            \
        const int rc__ = (call);                                                    \
        if(rc__ != SHQ_OK) {                                                        \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc__, last_error);             \
            return 1;                                                               \
        }                                                                           \
    } while(0)

static const double Box = 2 * M_PI;

/* raw sums of nb bins k = 2 .. 10 (every `skip`-th one empty) with delta_cdm = 1e-3 (a / 0.01) / (1 + k / 3) */
static std::vector<double> sums(int nb, double a, int skip)
{
    std::vector<double> s(3 * (size_t) nb + 1, 0.0);
    const double norm = 2.5;
    for(int i = 0; i < nb; i++) {
        const double k = 2 * pow(5.0, i / (nb - 1.0));
        const int64_t nm = skip && i % skip == 1 ? 0 : 3 + 2 * i;
        const double d = 1e-3 * (a / 0.01) / (1 + k / 3);
        s[i] = d * d * nm * norm / pow(Box, 3);
        s[nb + i] = k * nm;
        memcpy(&s[2 * (size_t) nb + i], &nm, sizeof(nm));
    }
    s[3 * (size_t) nb] = norm;
    return s;
}

static int run(Cosmo &c)
{
    c.OmegaNu1 = 0;
    for(int i = 0; i < 3; i++)
        c.OmegaNu1 += c.deg[i] * single0(&c, 1, i);
    std::vector<double> logk(20), tnu(20);
    for(int i = 0; i < 20; i++) {
        logk[i] = -3 + 6 * i / 19.0;
        tnu[i] = 0.4 / (1 + pow(pow(10, logk[i]) / 0.5, 2));
    }
    shq_nulra_params p = {};
    p.nk_allocated = 16;
    p.hybrid_enabled = c.hybrid;
    p.TimeTransfer = 0.01;
    p.TimeMax = 1;
    p.light = 299792;
    p.delta_nu_prefac = 1.5 * 0.2793 * c.H0 * c.H0 / p.light;
    p.OmegaNu1 = c.OmegaNu1;
    p.Omeganonu = 0.2793 - c.OmegaNu1;
    p.kBtnu = kBtnu;
    for(int i = 0; i < 3; i++) {
        p.mnu[i] = c.mnu[i];
        p.degeneracy[i] = c.deg[i];
        p.nufrac_low[i] = c.nufrac;
    }
    p.vcrit_by_light = 850.0 / 299792;
    p.nu_crit_time = c.crit;
    p.BoxSize_in_MPC = Box;
    p.NPowerTable = 20;
    p.logk = logk.data();
    p.T_nu = tnu.data();
    p.hubble = cb_hubble;
    p.omega_nu_nopart = cb_nopart;
    p.omega_nu_single = cb_single;
    p.user = &c;
    shq_nulra_host *h = nullptr, *g = nullptr;
    OK(shq_nulra_host_create(&p, &h));
    const double times[12] = {0.01, 0.012, 0.016, 0.022, 0.022, 0.035, 0.05, 0.052, 0.07, 0.1, 0.14, 0.2};
    for(double t : times)
        OK(shq_nulra_host_step(h, t, 0.01, sums(10, t, 0).data(), 10));
    shq_nulra_info info;
    std::vector<double> d(16), kk(16);
    OK(shq_nulra_host_download(h, d.data(), kk.data(), &info));
    if(info.ia != 8 || info.nk != 10 || info.kept != 1)
        return fprintf(stderr, "ia %d nk %d kept %d\n", info.ia, info.nk, info.kept), 1;
    /* the state into a second engine, then on both the rebin branch: 13 bins of which 9 carry modes, nk = 10 */
    shq_nulra_state st = {};
    OK(shq_nulra_host_get_state(h, &st));
    std::vector<double> sf(st.ia), dt((size_t) st.ia * st.nk), dni(st.nk), kv(st.nk), dnl(st.nk);
    st.scalefact = sf.data(); st.delta_tot = dt.data(); st.delta_nu_init = dni.data(); st.kvalue = kv.data(); st.delta_nu_last = dnl.data();
    OK(shq_nulra_host_get_state(h, &st));
    OK(shq_nulra_host_create(&p, &g));
    OK(shq_nulra_host_set_state(g, &st));
    const std::vector<double> s13 = sums(13, 0.3, 3);
    OK(shq_nulra_host_step(h, 0.3, 0.01, s13.data(), 13));
    OK(shq_nulra_host_step(g, 0.3, 0.01, s13.data(), 13));
    std::vector<double> d2(16);
    shq_nulra_info info2;
    OK(shq_nulra_host_download(h, d.data(), nullptr, &info));
    OK(shq_nulra_host_download(g, d2.data(), nullptr, &info2));
    if(info.nonzero == info.nk || info.ia != 9 || info2.ia != 9 || memcmp(d.data(), d2.data(), sizeof(double) * 10) != 0)
        return fprintf(stderr, "round trip: nonzero %d ia %d %d\n", info.nonzero, info.ia, info2.ia), 1;
    std::vector<double> T(193), T2(193);
    OK(shq_nulra_host_mode_table(h, 16, 1, T.data()));
    OK(shq_nulra_host_mode_table(g, 16, 1, T2.data()));
    if(memcmp(T.data(), T2.data(), sizeof(double) * 193) != 0 || !(T[1] > 1) || T[1] != T[3] || T[150] != T[192])
        return fprintf(stderr, "mode table\n"), 1;
    std::vector<double> dn(16);
    OK(shq_nulra_host_delta_nu(h, 0.3, dn.data()));
    for(int i = 0; i < 10; i++)
        if(!std::isfinite(dn[i]) || !std::isfinite(d[i]) || d[i] < 0)
            return fprintf(stderr, "delta_nu[%d] = %g %g\n", i, dn[i], d[i]), 1;
    printf("  hybrid %d: ia %d, %d nodes, delta_nu[0] %.17g, T[1] %.17g\n", c.hybrid, info.ia, info.nnodes, d[0], T[1]);
    shq_nulra_host_destroy(h);
    shq_nulra_host_destroy(g);
    return 0;
}

int main()
{
    Cosmo a = {0.1, {0.2, 0.05, 0.0}, {1, 1, 1}, 0, 0, 0, 0};
    Cosmo b = {100.0, {0.15, 0.15, 0.15}, {3, 0, 0}, 0, 0.3, 0.1, 1};
    if(run(a) || run(b))
        return 1;
    printf("nulra standalone ok\n");
    return 0;
}
