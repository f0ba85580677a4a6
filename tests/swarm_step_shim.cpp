// swarm_step_shim.cpp -- TEST ONLY.  One swarm step of PsoSolver::run() (psosolver.cpp:112-149, 286-306, 220-265) as the serial
// statements of the product compiled for the host: pso_move_particle (pais_dev.hpp) plus the fitness, gBest, inertia and
// convergence statements of pso_step_wave's serial form (pais_kernels.hip), on the swarm layout of pais_test_swarm_step
// (include/pais_test_hooks.h).  tests/test_swarm_step.py compares the GPU's lane-parallel step with it byte for byte;
// swarm_step_shim_main.cpp runs it under the sanitizers.  NOT a CPU fallback of the product.
#include <vector>

#include "../include/pais_test_hooks.h"
#include "../pais_mvs_amd/csrc/pais_dev.hpp"

extern "C" int shim_swarm_step(pais_test_swarm *s, double *swarm)
{
    const int N = s->n, maxIt = s->max_iteration;
    if (N < 1 || N > 128) return 1;
    std::vector<double> buf((size_t)14 * N);
    double(*pos)[3] = (double(*)[3])buf.data();
    double(*vec)[3] = pos + N;
    double(*pBest)[3] = vec + N;
    double(*nBest)[3] = pBest + N;
    double *fit = (double *)(nBest + N);
    double *pBestFit = fit + N;
    for (int i = 0; i < N; ++i) {
        for (int d = 0; d < 3; ++d) {
            pos[i][d] = swarm[14 * i + d];
            vec[i][d] = swarm[14 * i + 3 + d];
            pBest[i][d] = swarm[14 * i + 6 + d];
            nBest[i][d] = swarm[14 * i + 9 + d];
        }
        fit[i] = swarm[14 * i + 12];
        pBestFit[i] = swarm[14 * i + 13];
    }
    int it = s->iteration, g = s->g_idx;
    double gf = s->gbest_fitness, iw = s->iw;
    if (!s->started) {
        // initFitness (:112-119) + run(): gBest = particles[0].pBest; updateGbest (:137-149)
        for (int i = 0; i < N; ++i) pBestFit[i] = fit[i];
        g = 0;
        gf = pBestFit[0];
        for (int j = 0; j < N; ++j)
            if (pBestFit[j] <= gf) { gf = pBestFit[j]; g = j; }
        it = 0;
    } else {
        // updateFitness (:121-135): pBest on strict '<'
        for (int i = 0; i < N; ++i) {
            if (fit[i] < pBestFit[i]) {
                pBestFit[i] = fit[i];
                pBest[i][0] = pos[i][0];
                pBest[i][1] = pos[i][1];
                pBest[i][2] = pos[i][2];
            }
        }
        for (int j = 0; j < N; ++j)
            if (pBestFit[j] <= gf) { gf = pBestFit[j]; g = j; }
        const double niw = iw - 1.0 / maxIt; // :304
        iw = niw > 0.4 ? niw : 0.4;
        it += 1;
    }
    // loop head of run(): `iteration < maxIteration`, then the convergence break (:293-297)
    bool finished = it >= maxIt;
    if (!finished) {
        const double g0 = pBest[g][0], g1 = pBest[g][1], g2 = pBest[g][2];
        double disp = 0;
        for (int i = 0; i < N; ++i) {
            disp += fabs(pos[i][0] - g0);
            disp += fabs(pos[i][1] - g1);
            disp += fabs(pos[i][2] - g2);
        }
        disp /= (double)(3 * N);
        if (disp < 0.01) {
            double vel = 0;
            for (int i = 0; i < N; ++i) {
                vel += fabs(vec[i][0]);
                vel += fabs(vec[i][1]);
                vel += fabs(vec[i][2]);
            }
            vel /= (double)(3 * N);
            finished = vel < 0.01;
        }
    }
    if (finished) {
        s->continues = 0;
        s->result[0] = gf;
        s->result[1] = pBest[g][0];
        s->result[2] = pBest[g][1];
        s->result[3] = pBest[g][2];
        return 0;
    }
    // moveParticles (:220-265) for iteration `it`
    const double gB[3] = {pBest[g][0], pBest[g][1], pBest[g][2]};
    for (int i = 0; i < N; ++i) {
        double u[4];
        const uint32_t k0 = (uint32_t)(6 * N + 3 + 4 * (it * N + i));
        for (int q = 0; q < 4; ++q) u[q] = pais::uniform_from(s->stream_base, (uint32_t)s->run, k0 + q);
        pais::pso_move_particle(i, N, s->local_k, iw, u, pos, vec, pBest, nBest, fit, pBestFit, gB, s->range_l, s->range_u);
    }
    for (int i = 0; i < N; ++i) {
        for (int d = 0; d < 3; ++d) {
            swarm[14 * i + d] = pos[i][d];
            swarm[14 * i + 3 + d] = vec[i][d];
            swarm[14 * i + 6 + d] = pBest[i][d];
            swarm[14 * i + 9 + d] = nBest[i][d];
        }
        swarm[14 * i + 13] = pBestFit[i]; // (the fitness row is the evaluations': the step does not write it)
    }
    s->iteration = it;
    s->g_idx = g;
    s->gbest_fitness = gf;
    s->iw = iw;
    s->started = 1;
    s->continues = 1;
    return 0;
}
