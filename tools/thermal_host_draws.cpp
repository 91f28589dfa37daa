/* The host yardstick for shq_thermal_speeds: the draws of the reference's thermal-velocity loop as it runs them - ONE std::ranlux48,
 * reseeded at the start of every grid column, three outputs per particle along z - and nothing else (no interpolation, no
 * trigonometry), on one thread.  Prints one JSON line with the wall time.
 *
 *   g++ -O2 -std=c++17 tools/thermal_host_draws.cpp -o thermal_host_draws && ./thermal_host_draws 256 [columns]
 *
 * With a column count below Ngrid^2 only that many columns are run and the time is scaled up; the line says so. */
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char **argv)
{
    const long long ngrid = argc > 1 ? atoll(argv[1]) : 256;
    const long long all = ngrid * ngrid;
    long long ncol = argc > 2 ? atoll(argv[2]) : all;
    if(ngrid < 2 || ncol < 1)
        return 1;
    if(ncol > all)
        ncol = all;
    std::ranlux48 table(1), rng(0);
    uint64_t sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for(long long c = 0; c < ncol; c++) {
        rng.seed((uint32_t) table());
        for(long long z = 0; z < 3 * ngrid; z++)
            sum += rng();
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"ngrid\": %lld, \"columns_timed\": %lld, \"columns\": %lld, \"host_serial_draws_ms\": %.3f, \"host_serial_draws_ms_scaled\": %.3f, "
           "\"checksum\": %llu}\n",
           ngrid, ncol, all, ms, ms * (double) all / (double) ncol, (unsigned long long) sum);
    return 0;
}
