// pais_literal.hpp -- PAIS::getFitness (TMVS/mvs/patch.cpp:914-1047) in the REFERENCE'S OWN arithmetic: its per-pixel
// expressions and its summation order.  Selected with PAIS_ARITH=literal (round 6); device-only, included by pais_kernels.hip.
//
// The default evaluation (pais_eval.hpp, "kernel arithmetic") computes the same real-number function re-associated for a
// wave: the window origin once per run, fused multiply-adds in the homography rows, one reciprocal per camera pair,
// lerp-form bilinear taps, 1/K instead of /K, a polynomial exp, lane partial sums + butterflies.  Its values differ from the
// reference's in the last bits, and on a scene whose PSO runs do not converge a last-bit difference decides a
// `fitness < pBestFitness` the other way.  This file is the other end of that trade: one wave per
// evaluation as before, but
//   * the window from the particle's own centre (patch.cpp:944-962), x and y by the reference's repeated ++ (:979-980);
//   * per pixel and camera, in camIdx order (the reference camera at its own position, through its identity homography):
//     w = h6 x + h7 y + h8 without contraction, ix = (h0 x + h1 y + h2) / w with a true division (:994-996), the bounds
//     test of :999 on the doubles, the four-product bilinear of :1014-1017;
//   * mean /= K, avgSad /= K (:1022-1027), weight = 1 * dist * exp(-avgSad * avgSad / diffW) * exp(-1 / (edge * gradW)) in
//     that order (:1029-1038), with fdlibm's exp (det_exp: the platform libm of the reference's MSVC build is not
//     reproducible anywhere else; the CPU checker of the tests uses the same function);
//   * sumWeight += weight; fitness += weight * avgSad over the pixels in the reference's x-outer / y-inner order (:979-1041):
//     a wave computes 64 consecutive pixels of that order at a time and every lane adds the 64 (weight, weight * avgSad) one after
//     the other (v_readlane broadcasts) -- a strict sequential sum, bit for bit the CPU's.
// Checker: the CPU restatement's literal cost with the same exp / sin / cos (tests/test_gpu_parity.py:
// test_literal_arithmetic_cost_is_the_reference_statement).  Slower than the kernel arithmetic (a division per tap, two
// serial chains of S*S additions per evaluation); bench.py reports its throughput next to the default's.
#pragma once

// LDS of one evaluating wave: [EvalPatch][EvalCam x Kmax] [H: Kmax x 9] [colour rows: Kmax x 64] [w, wf: 2 x 64] [xs, ys: 2 x S]
// (S = 2 r + 1 <= 255: the walk's coordinates of every window column and row)
__host__ __device__ inline size_t literal_lds_bytes(int Kmax, int S)
{
    return eval_block_bytes(Kmax) + sizeof(double) * (9 * (size_t)Kmax + 64 * (size_t)Kmax + 2 * 64 + 2 * (size_t)S);
}

// What an evaluation reports besides its cost.  The PSO and fitness kernels take LitNoSink: every statement guarded by
// `if constexpr (Sink::on)` vanishes and their code is the one of the plain function.  pais_fitness_detail (k_fitness_detail)
// takes LitDetailSink: the per-pixel values of every 64-pixel trip, the homographies in camIdx order and the record, and a
// walk that goes on past an overflowing tap (the pixel is marked, the sums leave it out, the cost stays DBL_MAX).
struct LitNoSink {
    static constexpr bool on = false;
};
struct LitDetailSink {
    static constexpr bool on = true;
    pais_cost_detail *rec;
    double *weight, *avgSad; // S*S, walk order
    int8_t *code;            // S*S
    double *colour;          // K rows of S*S, or nullptr
    double *H;               // K x 9, or nullptr
};

// walk indices [from, S*S) carry no pixel (PAIS_PIX_NONE); lane 0 writes the record
__device__ void lit_detail_close(const LitDetailSink &dk, int from, int S2, int K, int lane, double value, double sumWeight, double fitness,
                                 const double *pt, int outcome, int nx, int ny, int live, int ovPix, int ovCam, int refPos)
{
    for (int k = from + lane; k < S2; k += 64) {
        dk.weight[k] = 0.0;
        dk.avgSad[k] = 0.0;
        dk.code[k] = PAIS_PIX_NONE;
        if (dk.colour)
            for (int i = 0; i < K; ++i) dk.colour[(size_t)i * S2 + k] = 0.0;
    }
    if (lane == 0) {
        pais_cost_detail r;
        r.fitness = value;
        r.sum_weight = sumWeight;
        r.sum_weighted_sad = fitness;
        r.pt[0] = pt[0];
        r.pt[1] = pt[1];
        r.outcome = outcome;
        r.nx = nx;
        r.ny = ny;
        r.live_pixels = live;
        r.overflow_pixel = ovPix;
        r.overflow_cam = ovCam;
        r.ref_pos = refPos;
        r._pad = 0;
        *dk.rec = r;
    }
}

// returns the cost of particle (theta, phi, depth); every lane gets the same value
template <class Sink = LitNoSink>
__device__ double eval_fitness_literal(const DevScene &sc, const EvalPatch *ep, const EvalCam *cams, double *Hbuf, double *crow, double *xs,
                                       double *ys, double *srow, double theta, double phi, double depth, int lane, const Sink &sink = Sink())
{
    double n[3];
    wave_spherical2normal(theta, phi, n, lane); // (the bits of det_sin / det_cos: utility.h:25-29 with the deterministic libm)
    {
        const double on[3] = {ep->optNref[0], ep->optNref[1], ep->optNref[2]};
        if (dot3(n, on) > 0) { // patch.cpp:939
            if constexpr (Sink::on) {
                const int S2 = sc.cfg.patchSize * sc.cfg.patchSize, K = ep->K;
                const double zero[2] = {0.0, 0.0};
                if (sink.H)
                    for (int q = lane; q < 9 * K; q += 64) sink.H[q] = 0.0; // (the reference returns before :948)
                lit_detail_close(sink, 0, S2, K, lane, DBL_MAX, 0.0, 0.0, zero, PAIS_COST_BACKFACING, 0, 0, 0, -1, -1,
                                 ep->hasRef ? ep->refPos : -1);
            }
            return DBL_MAX;
        }
    }
    const int K = ep->K, M = ep->M, LOD = ep->LOD, refCam = ep->refCam;
    const int refPos = ep->hasRef ? ep->refPos : -1; // position of the reference camera in camIdx (its first occurrence)
    const DevCamera &rc = sc.cams[refCam];
    double center[3];
    for (int i = 0; i < 3; ++i) center[i] = ep->ray[i] * depth + ep->Cref[i]; // :944
    // homographies of the other cameras (:290-330)
    {
        const double d = -dot3(center, n);
        double invH[9];
        ref_plane_inverse(d, ep->lodScale, ep->KRref, ep->KTref, n, invH);
        for (int c = lane; c < M; c += 64) {
            double H[9];
            patch_homography(cams[c].cam == refCam, d, ep->lodScale, cams[c].KR, cams[c].KT, n, invH, H);
            for (int i = 0; i < 9; ++i) Hbuf[c * 9 + i] = H[i];
        }
    }
    if constexpr (Sink::on) { // H in camIdx order: the identity at refPos, camera i > refPos in slot i - 1
        wave_sync();
        if (sink.H)
            for (int q = lane; q < 9 * K; q += 64) {
                const int i = q / 9, j = q - 9 * i;
                sink.H[q] = i == refPos ? ((j & 3) == 0 ? 1.0 : 0.0) : Hbuf[9 * (i - (refPos >= 0 && i > refPos ? 1 : 0)) + j];
            }
    }
    // the particle's own window (:952-962)
    const int refW = rc.w[LOD], refH = rc.h[LOD];
    const int r = sc.cfg.patchRadius, S = sc.cfg.patchSize;
    double pt[2];
    project_raw(rc.R, rc.T, rc.focal, rc.pp, ep->lodScale, center, pt);
    if constexpr (Sink::on) {
        const int outcome = !(LOD <= rc.maxLOD && in_image_d(pt, refW, refH)) ? PAIS_COST_OFF_IMAGE
                            : (pt[0] - r < 2 || pt[0] + r >= refW - 3 || pt[1] - r < 2 || pt[1] + r >= refH - 3) ? PAIS_COST_WINDOW
                                                                                                               : PAIS_COST_OK;
        if (outcome != PAIS_COST_OK) {
            lit_detail_close(sink, 0, S * S, K, lane, DBL_MAX, 0.0, 0.0, pt, outcome, 0, 0, 0, -1, -1, refPos);
            return DBL_MAX;
        }
    }
    if (!(LOD <= rc.maxLOD && in_image_d(pt, refW, refH))) return DBL_MAX;                                     // :952
    if (pt[0] - r < 2 || pt[0] + r >= refW - 3 || pt[1] - r < 2 || pt[1] + r >= refH - 3) return DBL_MAX;       // :957-962
    // x and y of the walk: start + 1 + 1 + ... (:979-980), by one lane; at most S values of either (the distance table has S x S,
    // xs and ys have S entries)
    int nx = 0, ny = 0;
    {
        wave_sync();
        if (lane == 0) {
            int k = 0;
            for (double x = pt[0] - r; x <= pt[0] + r && k < S; ++x) xs[k++] = x;
            srow[0] = (double)k;
        } else if (lane == 1) {
            int k = 0;
            for (double y = pt[1] - r; y <= pt[1] + r && k < S; ++y) ys[k++] = y;
            srow[1] = (double)k;
        }
        wave_sync();
        nx = (int)srow[0];
        ny = (int)srow[1];
    }
    const uint8_t *refImg = sc.imgBlob + rc.imgOff[LOD];
    const double *refEdge = sc.edgeBlob ? sc.edgeBlob + rc.edgeOff[LOD] : nullptr;
    const double eMin = rc.edgeMin[LOD], eMax = rc.edgeMax[LOD];
    const bool useDist = sc.cfg.adaptiveDistanceEnable != 0, useDiff = sc.cfg.adaptiveDifferenceEnable != 0,
               useGrad = sc.cfg.adaptiveGradientEnable != 0;
    const double diffW = sc.cfg.diffWeighting, gradW = sc.cfg.gradientWeighting;
    double *myc = crow + lane;
    double fitness = 0, sumWeight = 0;
    const int total = nx * ny;
    int nLive = 0, ovPix = -1, ovCam = -1; // (LitDetailSink)
    for (int k0 = 0; k0 < total; k0 += 64) {
        const int k = k0 + lane;
        const bool have = k < total;
        const int kk = have ? k : 0;
        const int xi = kk / ny, yi = kk - xi * ny;
        const double x = xs[xi], y = ys[yi];
        const int rx = cv_round(x), ry = cv_round(y);
        const bool live = have && refImg[(size_t)ry * refW + rx] != 0; // :986 (a masked pixel is skipped before any tap)
        bool over = false;
        double mean = 0;
        int slot = 0;
        int firstBad = -1; // (LitDetailSink) the lane's first camera with a bad tap
        for (int i = 0; i < K; ++i) {
            const bool isRef = (i == refPos); // wave-uniform
            const uint8_t *img;
            int cols, rows;
            double w, ix, iy;
            if (isRef) { // the identity homography (:317-320) through the same expressions
                img = refImg; cols = refW; rows = refH;
                w = (0.0 * x + 0.0 * y + 1.0);
                ix = (1.0 * x + 0.0 * y + 0.0) / w;
                iy = (0.0 * x + 1.0 * y + 0.0) / w;
            } else {
                const double *Hi = Hbuf + 9 * slot;
                img = sc.imgBlob + cams[slot].imgOff; cols = cams[slot].w; rows = cams[slot].h;
                w = (Hi[6] * x + Hi[7] * y + Hi[8]);           // :994
                ix = (Hi[0] * x + Hi[1] * y + Hi[2]) / w;      // :995
                iy = (Hi[3] * x + Hi[4] * y + Hi[5]) / w;      // :996
                ++slot;
            }
            const bool bad = ix < 2 || ix >= cols - 3 || iy < 2 || iy >= rows - 3 || w == 0 || ix != ix || iy != iy; // :999
            over = over || bad;
            if constexpr (Sink::on) firstBad = (bad && firstBad < 0) ? i : firstBad;
            const bool tap = live && !bad;
            const int px0 = tap ? (int)ix : 2, py0 = tap ? (int)iy : 2; // (an address inside the level for the lanes that do not count)
            const int px1 = px0 + 1, py2 = py0 + 1;
            const uint8_t *r0 = img + (size_t)py0 * cols + px0, *r1 = r0 + cols;
            const double c = (double)r0[0] * (px1 - ix) * (py2 - iy) + (double)r0[1] * (ix - px0) * (py2 - iy) +
                             (double)r1[0] * (px1 - ix) * (iy - py0) + (double)r1[1] * (ix - px0) * (iy - py0); // :1014-1017
            myc[i * 64] = c;
            mean += c;
        }
        if constexpr (Sink::on) { // the walk goes on: the first overflowing pixel and its camera are recorded
            const unsigned long long ob = __ballot(live && over);
            if (ob && ovPix < 0) {
                const int j = __ffsll((long long)ob) - 1;
                ovPix = k0 + j;
                ovCam = __shfl(firstBad, j, 64);
            }
        } else {
            if (__any(live && over)) return DBL_MAX; // :1001 -- whole call
        }
        mean /= K;                                // :1022
        double avgSad = 0;
        for (int i = 0; i < K; ++i) avgSad += fabs(myc[i * 64] - mean);
        avgSad /= K;                              // :1027
        double weight = 1;
        if (useDist) weight *= sc.gauss[kk];      // :1031 (the table iterator advances once per pixel of the walk: index k)
        if (useDiff) weight *= det_exp(-avgSad * avgSad / diffW); // :1034
        if (useGrad) {
            const double e = refEdge ? refEdge[(size_t)ry * refW + rx] : edge_on_the_fly(refImg, refW, refH, rx, ry, eMin, eMax);
            weight *= det_exp(-1.0 / (e * gradW)); // :1037
        }
        // the 64 pixels of this trip, added in the reference's order by every lane alike: lane j's (weight, weight * avgSad) are
        // broadcast with v_readlane (an SGPR lane index: no LDS round trip inside the two serial chains of additions)
        const double wf = weight * avgSad;
        bool counted = live;
        if constexpr (Sink::on) counted = live && !over;
        unsigned long long todo = __ballot(counted);
        if constexpr (Sink::on) { // this trip's 64 walk indices: coalesced stores of the maps, the colours one camera row at a time
            const int S2 = S * S;
            nLive += __popcll(todo);
            if (k < S2) {
                const double nan = __builtin_nan("");
                const int8_t cd = !have ? PAIS_PIX_NONE : (!live ? PAIS_PIX_MASKED : (over ? PAIS_PIX_OVERFLOW : PAIS_PIX_COUNTED));
                sink.weight[k] = cd == PAIS_PIX_COUNTED ? weight : (cd == PAIS_PIX_OVERFLOW ? nan : 0.0);
                sink.avgSad[k] = cd == PAIS_PIX_COUNTED ? avgSad : (cd == PAIS_PIX_OVERFLOW ? nan : 0.0);
                sink.code[k] = cd;
                if (sink.colour)
                    for (int i = 0; i < K; ++i)
                        sink.colour[(size_t)i * S2 + k] = cd == PAIS_PIX_COUNTED ? myc[i * 64] : (cd == PAIS_PIX_OVERFLOW ? nan : 0.0);
            }
        }
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            sumWeight += lane_get(weight, j); // :1040
            fitness += lane_get(wf, j);       // :1041
        }
    }
    if constexpr (Sink::on) {
        const double value = ovPix >= 0 ? DBL_MAX : fitness / sumWeight;
        const int outcome = ovPix >= 0 ? PAIS_COST_OVERFLOW : (nLive == 0 ? PAIS_COST_ALL_MASKED : PAIS_COST_OK);
        lit_detail_close(sink, (total + 63) & ~63, S * S, K, lane, value, sumWeight, fitness, pt, outcome, nx, ny, nLive, ovPix, ovCam,
                         refPos);
        return value;
    }
    return fitness / sumWeight; // :1046 (NaN when every pixel was masked)
}

// pais_fitness_batch in the literal arithmetic: one wave (= one workgroup) per evaluation
__global__ __launch_bounds__(64) void k_fitness_lit(DevScene sc, const int32_t *stateIndex, const double *particles, double *out, int nEvals,
                                                    int Kmax, const unsigned char *evalBlocks, size_t evalBlockBytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *crow = Hbuf + 9 * (size_t)Kmax, *srow = crow + 64 * (size_t)Kmax, *xs = srow + 2 * 64, *ys = xs + sc.cfg.patchSize;
    const int lane = threadIdx.x;
    const int nw = (int)(eval_block_bytes(Kmax) / 8);
    for (int e = blockIdx.x; e < nEvals; e += gridDim.x) {
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)stateIndex[e]);
        wave_sync();
        for (int q = lane; q < nw; q += 64) ((uint64_t *)smem)[q] = src[q];
        wave_sync();
        const double v = eval_fitness_literal(sc, ep, cams, Hbuf, crow, xs, ys, srow, particles[3 * e], particles[3 * e + 1], particles[3 * e + 2], lane);
        if (lane == 0) out[e] = v;
    }
}

// pais_fitness_detail: k_fitness_lit with LitDetailSink -- the same cost, and per evaluation the record, the S x S maps of
// weight, avgSad and pixel code, and optionally the colours (Kmax rows of S x S) and homographies (Kmax x 9)
__global__ __launch_bounds__(64) void k_fitness_detail(DevScene sc, const int32_t *stateIndex, const double *particles, int nEvals, int Kmax,
                                                       const unsigned char *evalBlocks, size_t evalBlockBytes, pais_cost_detail *rec,
                                                       double *weight, double *avgSad, int8_t *code, double *colour, double *H)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *crow = Hbuf + 9 * (size_t)Kmax, *srow = crow + 64 * (size_t)Kmax, *xs = srow + 2 * 64, *ys = xs + sc.cfg.patchSize;
    const int lane = threadIdx.x;
    const int nw = (int)(eval_block_bytes(Kmax) / 8);
    const size_t S2 = (size_t)sc.cfg.patchSize * sc.cfg.patchSize;
    for (int e = blockIdx.x; e < nEvals; e += gridDim.x) {
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)stateIndex[e]);
        wave_sync();
        for (int q = lane; q < nw; q += 64) ((uint64_t *)smem)[q] = src[q];
        wave_sync();
        LitDetailSink dk;
        dk.rec = rec + e;
        dk.weight = weight + S2 * e;
        dk.avgSad = avgSad + S2 * e;
        dk.code = code + S2 * e;
        dk.colour = colour ? colour + S2 * Kmax * e : nullptr;
        dk.H = H ? H + (size_t)9 * Kmax * e : nullptr;
        eval_fitness_literal(sc, ep, cams, Hbuf, crow, xs, ys, srow, particles[3 * e], particles[3 * e + 1], particles[3 * e + 2], lane, dk);
    }
}

// the evaluation launch of a PSO iteration in the literal arithmetic: one wave per (candidate, particle) -- the interface of
// k_pso_eval2; k_pso_step follows it as in the large-batch pipeline
__global__ __launch_bounds__(64) void k_pso_eval_lit(DevScene sc, unsigned char *states, int n, int Nmax, int Kmax, const unsigned char *evalBlocks,
                                                     size_t evalBlockBytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *crow = Hbuf + 9 * (size_t)Kmax, *srow = crow + 64 * (size_t)Kmax, *xs = srow + 2 * 64, *ys = xs + sc.cfg.patchSize;
    const int lane = threadIdx.x;
    const size_t SB = pso_state_bytes(Nmax);
    const int total = n * Nmax;
    const int nw = (int)(eval_block_bytes(Kmax) / 8);
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int c = t / Nmax, i = t - c * Nmax;
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        PsoArrays A = pso_arrays((unsigned char *)hd, Nmax);
        if (!hd->active || i >= hd->N) continue;
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)c);
        wave_sync();
        for (int q = lane; q < nw; q += 64) ((uint64_t *)smem)[q] = src[q];
        wave_sync();
        const double v = eval_fitness_literal(sc, ep, cams, Hbuf, crow, xs, ys, srow, A.pos[i][0], A.pos[i][1], A.pos[i][2], lane);
        if (lane == 0) A.fit[i] = v;
    }
}
