// rdf_moments_math.h — the formulas of rdf_moments / rdf_comoments / rdf_groupby_moments: the ONE definition of the merge of
// two moment states, of a tile's finish and of the statistics read off a state.  The kernels fold their tile states with
// it (rdf_moments.hip, rdf_group_moments.hip), the host folds the blocks' states with it, rdf_moments_merge and
// rdf_moments_stat hand it to callers.  Host and device are compiled -ffp-contract=off, so the formulas round the same way
// on both.  __host__ __device__ inline under hipcc; plain g++ compiles it into tests/cpp/test_group_moments_host.cpp: it
// includes nothing of HIP.
#pragma once
#include <stdint.h>

#include "../../include/rdf_mi355x.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_MO_HD __host__ __device__ inline
#else
#define RDF_MO_HD inline
#endif

// s + e = a + b exactly (Knuth's two-sum: no ordering of |a|, |b| assumed)
RDF_MO_HD void mo_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// mean (hi, lo) <- (hi, lo) + t, renormalised so that |lo| <= ulp(hi) / 2
RDF_MO_HD void mo_mean_add(double& hi, double& lo, double t) {
    double s, e;
    mo_two_sum(hi, t, s, e);
    e += lo;
    hi = s + e;
    lo = e - (hi - s);
}

// Chan / Pebay: the state of the rows of a and b together.  delta between the two double-double means is known to an ulp
// of delta, not of the means; one division, the rest multiplications and additions.
RDF_MO_HD void mo_merge(rdf_moments_state& a, const rdf_moments_state& b) {
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

RDF_MO_HD void mo_comerge(rdf_comoments_state& a, const rdf_comoments_state& b) {
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
RDF_MO_HD rdf_moments_state mo_tile_state(int64_t n, double c, double s1, double s2, double s3, double s4) {
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
RDF_MO_HD rdf_comoments_state mo_cotile_state(int64_t n, double cx, double cy, double sx, double sy, double sxx, double syy, double sxy) {
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

// The statistics read off a state: ONE definition for rdf_moments_stat / rdf_comoments_stat on the host and for the finish
// kernel of rdf_groupby_moments on the device.  -> false: the statistic is absent (no rows, a sample form of one row, a
// ratio over M2 == 0) and *out is left alone.  stat is a valid rdf_stat / rdf_costat.
RDF_MO_HD bool mo_stat(const rdf_moments_state& s, int32_t stat, double* out) {
    const double n = (double)s.count;
    const bool samp = stat == RDF_STAT_VAR_SAMP || stat == RDF_STAT_STDDEV_SAMP;
    if (s.count <= 0 || (samp && s.count < 2)) return false;
    if ((stat == RDF_STAT_SKEWNESS || stat == RDF_STAT_KURTOSIS) && s.m2 == 0.0) return false;
    switch (stat) {
        case RDF_STAT_MEAN: *out = s.mean + s.mean_lo; break;
        case RDF_STAT_VAR_POP: *out = s.m2 / n; break;
        case RDF_STAT_VAR_SAMP: *out = s.m2 / (n - 1.0); break;
        case RDF_STAT_STDDEV_POP: *out = __builtin_sqrt(s.m2 / n); break;
        case RDF_STAT_STDDEV_SAMP: *out = __builtin_sqrt(s.m2 / (n - 1.0)); break;
        case RDF_STAT_SKEWNESS: *out = __builtin_sqrt(n) * s.m3 / (s.m2 * __builtin_sqrt(s.m2)); break;
        default: *out = n * s.m4 / (s.m2 * s.m2) - 3.0; break;
    }
    return true;
}
RDF_MO_HD bool mo_costat(const rdf_comoments_state& s, int32_t stat, double* out) {
    const double n = (double)s.count;
    if (s.count <= 0 || (stat == RDF_COSTAT_COVAR_SAMP && s.count < 2)) return false;
    if (stat == RDF_COSTAT_CORR && (s.m2x == 0.0 || s.m2y == 0.0)) return false;
    switch (stat) {
        case RDF_COSTAT_COVAR_POP: *out = s.cxy / n; break;
        case RDF_COSTAT_COVAR_SAMP: *out = s.cxy / (n - 1.0); break;
        default: *out = s.cxy / __builtin_sqrt(s.m2x * s.m2y); break;
    }
    return true;
}
