// rdf_moments.h — rdf_moments / rdf_comoments (kernels: rdf_moments.hip, host side: rdf_capi_moments.inc): the argument
// block, the launchers, and the ONE definition of the merge of two moment states — the kernel folds its tile states with
// it, the host folds the blocks' states with it, and rdf_moments_merge hands it to callers.  Host and device are compiled
// -ffp-contract=off, so the formulas round the same way on both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_colstats.h"

// s + e = a + b exactly (Knuth's two-sum: no ordering of |a|, |b| assumed)
__host__ __device__ inline void mo_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// mean (hi, lo) <- (hi, lo) + t, renormalised so that |lo| <= ulp(hi) / 2
__host__ __device__ inline void mo_mean_add(double& hi, double& lo, double t) {
    double s, e;
    mo_two_sum(hi, t, s, e);
    e += lo;
    hi = s + e;
    lo = e - (hi - s);
}

// Chan / Pebay: the state of the rows of a and b together.  delta between the two double-double means is known to an ulp
// of delta, not of the means; one division, the rest multiplications and additions.
__host__ __device__ inline void mo_merge(rdf_moments_state& a, const rdf_moments_state& b) {
    if (b.count == 0) return;
    if (a.count == 0) { a = b; return; }
    const double na = (double)a.count, nb = (double)b.count;
    const double inv = 1.0 / (na + nb), fa = na * inv, fb = nb * inv;
    const double d = (b.mean - a.mean) + (b.mean_lo - a.mean_lo);
    const double d2 = d * d, w = na * fb;   // na nb / n
    const double m4 = (a.m4 + b.m4) + ((d2 * d2) * (w * ((fa * fa - fa * fb) + fb * fb)) + (6.0 * d2) * (fa * fa * b.m2 + fb * fb * a.m2) +
                                       (4.0 * d) * (fa * b.m3 - fb * a.m3));
    const double m3 = (a.m3 + b.m3) + ((d2 * d) * (w * (fa - fb)) + (3.0 * d) * (fa * b.m2 - fb * a.m2));
    const double m2 = (a.m2 + b.m2) + d2 * w;
    mo_mean_add(a.mean, a.mean_lo, d * fb);
    a.count += b.count;
    a.m2 = m2; a.m3 = m3; a.m4 = m4;
}

__host__ __device__ inline void mo_comerge(rdf_comoments_state& a, const rdf_comoments_state& b) {
    if (b.count == 0) return;
    if (a.count == 0) { a = b; return; }
    const double na = (double)a.count, nb = (double)b.count;
    const double inv = 1.0 / (na + nb), fb = nb * inv, w = na * fb;
    const double dx = (b.mean_x - a.mean_x) + (b.mean_x_lo - a.mean_x_lo);
    const double dy = (b.mean_y - a.mean_y) + (b.mean_y_lo - a.mean_y_lo);
    a.m2x = (a.m2x + b.m2x) + (dx * dx) * w;
    a.m2y = (a.m2y + b.m2y) + (dy * dy) * w;
    a.cxy = (a.cxy + b.cxy) + (dx * dy) * w;
    mo_mean_add(a.mean_x, a.mean_x_lo, dx * fb);
    mo_mean_add(a.mean_y, a.mean_y_lo, dy * fb);
    a.count += b.count;
}

// A tile's power sums about its centre c -> its state.  s1..s4 = sum d^k with d = x - c over the n counted rows (n > 0):
// the true mean is c + e with e = s1 / n, and the central sums follow from the binomial expansion of (d - e)^k.
__host__ __device__ inline rdf_moments_state mo_tile_state(int64_t n, double c, double s1, double s2, double s3, double s4) {
    const double nd = (double)n, e = s1 / nd, e2 = e * e;
    rdf_moments_state t;
    t.count = n;
    t.mean = c; t.mean_lo = 0.0;
    mo_mean_add(t.mean, t.mean_lo, e);
    t.m2 = s2 - nd * e2;
    t.m3 = (s3 - (3.0 * e) * s2) + (2.0 * nd) * (e2 * e);
    t.m4 = ((s4 - (4.0 * e) * s3) + (6.0 * e2) * s2) - (3.0 * nd) * (e2 * e2);
    return t;
}
__host__ __device__ inline rdf_comoments_state mo_cotile_state(int64_t n, double cx, double cy, double sx, double sy, double sxx, double syy, double sxy) {
    const double nd = (double)n, ex = sx / nd, ey = sy / nd;
    rdf_comoments_state t;
    t.count = n;
    t.mean_x = cx; t.mean_x_lo = 0.0;
    t.mean_y = cy; t.mean_y_lo = 0.0;
    mo_mean_add(t.mean_x, t.mean_x_lo, ex);
    mo_mean_add(t.mean_y, t.mean_y_lo, ey);
    t.m2x = sxx - nd * (ex * ex);
    t.m2y = syy - nd * (ey * ey);
    t.cxy = sxy - nd * (ex * ey);
    return t;
}

// A wave's tile: 64 lanes x kMoRowsPerLane rows; the four waves of a block share one tile of CsCol (kCsTile rows of one chunk).
constexpr int kMoRowsPerLane = 8;
constexpr int kMoWaveTile = 64 * kMoRowsPerLane;
static_assert(kMoWaveTile * (kCsThreads / 64) == kCsTile, "a block's four wave tiles make one tile of CsCol");

struct MoArgs {
    CsCol    col;                   // x: chunks, row and tile prefix tables
    const rdfk::DevChunkCol* y;     // [nchunks] rdf_comoments, else nullptr
    const rdfk::DevChunkCol* mask;  // [nchunks] RDF_BOOL chunks (values = the bits), or nullptr
    int32_t  dt_x, dt_y;            // rdf_dtype
    void*    out;                   // [grid] rdf_moments_state / rdf_comoments_state, one per block
};

int        mo_grid(int64_t ntiles);
hipError_t launch_mo_moments(const MoArgs& a, int grid, hipStream_t s);
hipError_t launch_mo_comoments(const MoArgs& a, int grid, hipStream_t s);
