/* sfr_host_main.cpp — a stand-alone program for the host sanitizers (no python, no GPU): csrc/sfr_host.hip and csrc/cooling_host.hip
 * with the one function they need of the rest of the library, and a main that runs shq_sfr_eval_host over a dump of the tests'
 * particle set (tests/sfr_cases.py: dump(); the dense set and the edge rows under the global UVBG and under the synthetic net-heating
 * one) and compares every output with the results recorded in the dump, bit for bit.
 *
 *     hipcc --offload-host-only -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
 *         shenqi_amd/csrc/cooling_host.hip shenqi_amd/csrc/sfr_host.hip tools/sfr_host_main.cpp -o sfr_host_check -lpthread
 *     python -c "import sys; sys.path[:0] = ['.', 'tests']; import sfr_cases; sfr_cases.dump('sfr.dump')" && ./sfr_host_check sfr.dump */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "shenqi_hip.h"

static char last_error[1024];
void shq_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if(argc < 2) {
        fprintf(stderr, "usage: %s dump\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if(!f) {
        perror(argv[1]);
        return 2;
    }
    int64_t hdr[3]; /* n, random table size, parameter sets */
    shq_cooling_tables tab;
    std::vector<double> rates(14 * SHQ_COOL_NRECOMBTAB);
    shq_sfr_eval_step step;
    if(!rd(f, hdr, 3) || !rd(f, &tab, 1) || !rd(f, rates.data(), rates.size()) || !rd(f, &step, 1))
        return 2;
    const size_t n = (size_t) hdr[0], nrnd = (size_t) hdr[1];
    std::vector<double> rnd(nrnd), d[11];
    std::vector<uint8_t> timebin(n), flags(n);
    std::vector<uint64_t> id(n);
    bool ok = rd(f, rnd.data(), nrnd);
    for(auto &v : d) {
        v.resize(n);
        ok = ok && rd(f, v.data(), n);
    }
    ok = ok && rd(f, timebin.data(), n) && rd(f, flags.data(), n) && rd(f, id.data(), n);
    if(!ok)
        return 2;
    tab.rate_tables = rates.data();
    tab.metal = NULL;
    tab.zreion = NULL;
    step.rnd_table = rnd.data();
    const shq_sfr_arrays in = {d[0].data(), d[1].data(), d[2].data(), d[3].data(), d[4].data(), d[5].data(), d[6].data(),
                               d[7].data(), d[8].data(), d[9].data(), d[10].data(), timebin.data(), flags.data(), id.data()};
    int bad = 0;
    for(int64_t s = 0; s < hdr[2]; s++) {
        shq_sfr_params par;
        int32_t what;
        shq_cooling_uvbg local;
        std::vector<double> want((size_t) SHQ_SFR_NOUT * n), out((size_t) SHQ_SFR_NOUT * n, 0.0);
        std::vector<uint8_t> wb(3 * n), b(3 * n, 0);
        std::vector<int32_t> wi(2 * n), st(n, 0), steps(n, 0);
        if(!rd(f, &par, 1) || !rd(f, &local, 1) || !rd(f, &what, 1) || !rd(f, want.data(), want.size()) || !rd(f, wb.data(), wb.size()) || !rd(f, wi.data(), wi.size()))
            return 2;
        step.LocalUVBG = local;
        for(int threads = 1; threads <= 4; threads += 3) {
            const int rc = shq_sfr_eval_host(&tab, &par, what, (int64_t) n, &in, &step, out.data(), b.data(), b.data() + n, b.data() + 2 * n, st.data(), steps.data(), threads);
            if(rc != SHQ_OK) {
                fprintf(stderr, "set %ld: rc %d: %s\n", (long) s, rc, last_error);
                return 1;
            }
            size_t nok = 0, diff = 0;
            for(size_t k = 0; k < n; k++) {
                diff += st[k] != wi[k] || steps[k] != wi[n + k];
                if(st[k] != SHQ_COOL_OK)
                    continue;
                nok++;
                for(size_t r = 0; r < SHQ_SFR_NOUT; r++)
                    diff += memcmp(&out[r * n + k], &want[r * n + k], sizeof(double)) != 0;
                diff += b[k] != wb[k] || b[n + k] != wb[n + k] || b[2 * n + k] != wb[2 * n + k];
            }
            printf("set %ld (what %d, BHFeedbackUseTcool %d, criterion %d, epsH0 %g), %d thread(s): %zu particles, %zu OK, %zu differences\n", (long) s, (int) what,
                   (int) par.BHFeedbackUseTcool, (int) par.StarformationCriterion, local.epsH0, threads, n, nok, diff);
            bad += diff != 0;
        }
    }
    fclose(f);
    /* the argument checks: a NULL GradRho with the H2 bits, Generations < 1 */
    shq_sfr_params par;
    memset(&par, 0, sizeof(par));
    par.Generations = 0;
    std::vector<double> out((size_t) SHQ_SFR_NOUT * n);
    std::vector<uint8_t> b(3 * n);
    std::vector<int32_t> st(n);
    bad += shq_sfr_eval_host(&tab, &par, 0, (int64_t) n, &in, &step, out.data(), b.data(), b.data() + n, b.data() + 2 * n, st.data(), NULL, 1) != SHQ_ERR_INVALID;
    par.Generations = 2;
    par.StarformationCriterion = 3;
    shq_sfr_arrays nograd = in;
    nograd.GradRho = NULL;
    bad += shq_sfr_eval_host(&tab, &par, 0, (int64_t) n, &nograd, &step, out.data(), b.data(), b.data() + n, b.data() + 2 * n, st.data(), NULL, 1) != SHQ_ERR_INVALID;
    printf(bad ? "FAILED\n" : "all equal\n");
    return bad ? 1 : 0;
}
