// swarm_step_shim_main.cpp -- TEST ONLY.  Stand-alone driver of swarm_step_shim.cpp for the sanitizers (address, undefined):
// the degenerate swarms of tests/test_swarm_step.py (NaN and +inf fitness among them) at every swarm size, several steps each.
// Prints the number of steps run.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/pais_test_hooks.h"

extern "C" int shim_swarm_step(pais_test_swarm *s, double *swarm);

static unsigned long long lcg(unsigned long long &x) { return x = x * 6364136223846793005ULL + 1442695040888963407ULL; }
static double unit(unsigned long long &x) { return (double)(lcg(x) >> 11) / 9007199254740992.0; }

int main()
{
    unsigned long long x = 42;
    long steps = 0;
    for (int N = 1; N <= 128; N += (N < 20 ? 1 : 15)) {
        // kinds 6, 7, 8: NaN fitness among finite ones, every fitness NaN, +inf among finite ones
        for (int kind = 0; kind < 9; ++kind) {
            for (int started = 0; started < 2; ++started) {
                pais_test_swarm s;
                memset(&s, 0, sizeof(s));
                const double lo[3] = {0.5, -1.0, 2.0}, hi[3] = {1.5, 1.0, 4.0};
                for (int d = 0; d < 3; ++d) { s.range_l[d] = lo[d]; s.range_u[d] = hi[d]; }
                s.n = N; s.max_iteration = 30; s.iteration = started ? 2 : 0; s.started = started; s.run = 1;
                s.local_k = N < 5 ? N : 5; s.iw = 0.7; s.stream_base = lcg(x); s.g_idx = 0;
                std::vector<double> sw((size_t)14 * N);
                for (int i = 0; i < N; ++i) {
                    double *r = &sw[(size_t)14 * i];
                    for (int d = 0; d < 3; ++d) {
                        r[d] = lo[d] + (hi[d] - lo[d]) * unit(x);
                        r[3 + d] = 0.2 * (unit(x) - 0.5);
                        r[6 + d] = kind == 0 ? 0.5 * (lo[d] + hi[d]) : lo[d] + (hi[d] - lo[d]) * unit(x);
                        r[9 + d] = r[6 + d];
                        if (kind == 1) r[d] = r[6 + d] = hi[d];
                        if (kind == 4) r[d] = r[6 + d];
                    }
                    r[12] = kind == 2 ? DBL_MAX : 5.0 * unit(x);
                    r[13] = kind == 2 ? DBL_MAX : (kind == 3 ? 1.0 : 5.0 * unit(x));
                    if (kind == 6 && i % 3 == 0) r[12] = r[13] = NAN;
                    if (kind == 7) r[12] = r[13] = NAN;
                    if (kind == 8 && i % 2 == 0) r[12] = INFINITY;
                }
                s.gbest_fitness = sw[13];
                for (int t = 0; t < 4; ++t) {
                    if (shim_swarm_step(&s, sw.data()) != 0) return 1;
                    ++steps;
                    if (!s.continues) break;
                    for (int i = 0; i < N; ++i) {
                        double f = kind == 2 ? DBL_MAX : 5.0 * unit(x);
                        if ((kind == 6 && (i + t) % 3 == 0) || kind == 7) f = NAN;
                        if (kind == 8 && (i + t) % 2 == 0) f = INFINITY;
                        sw[(size_t)14 * i + 12] = f;
                    }
                }
            }
        }
    }
    printf("%ld steps\n", steps);
    return steps > 0 ? 0 : 1;
}
