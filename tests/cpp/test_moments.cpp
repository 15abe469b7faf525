// AggregateFunctions::variance / stddev / var_pop / stddev_pop / skewness / kurtosis and corr / covar_pop / covar_samp in
// the C++ mirror (rdf_frame.hpp -> rdf_moments / rdf_comoments), run on the device over uk_cities_with_headers.csv.  The
// answers are the exact ones of tests/moments_ref.py rounded to double, the tolerances its bounds (B = gamma(2n) + 16u at
// n = 37, relative to the statistic: 9.99e-15 for the variances, 1.42e-14 for the skewness, 4.6e-14 for the kurtosis, 1.34e-14
// for covariances and corr; at the 12 masked rows 4.44e-15 and 9.5e-15), written out as constants and rounded down.
#include <cmath>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using AGG = AggregateFunctions;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

TEST(moments_of_lat) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const ChunkedArray& lat = df.column_by_name("lat").data();
    CHECK_NEAR(*AGG::variance(lat), 3.6793042009666967, 9.99e-15);
    CHECK_NEAR(*AGG::stddev(lat), 1.9181512455921448, 9.99e-15);
    CHECK_NEAR(*AGG::var_pop(lat), 3.5798635468865156, 9.99e-15);
    CHECK_NEAR(*AGG::stddev_pop(lat), 1.8920527336431496, 9.99e-15);
    CHECK_NEAR(*AGG::skewness(lat), 1.2484246678618836, 1.42e-14);
    CHECK_NEAR(*AGG::kurtosis(lat), 0.830770544609576, 4.6e-14);
    const AGG::Moments m = AGG::moments(lat);
    CHECK_EQ(m.count(), (int64_t)37);
    CHECK_NEAR(*m.stat(RDF_STAT_MEAN), 52.65178643243243, 4.2e-15);
    CHECK_EQ(*m.stat(RDF_STAT_VAR_SAMP), *AGG::variance(lat));      // the same input gives the same bytes
    CHECK_EQ(*AGG::avg(lat) > 52.0, true);
}

TEST(corr_of_lat_and_lng) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const ChunkedArray& lat = df.column_by_name("lat").data();
    const ChunkedArray& lng = df.column_by_name("lng").data();
    CHECK_NEAR(*AGG::corr(lat, lng), -0.5262228251289963, 1.34e-14);
    CHECK_NEAR(*AGG::covar_pop(lat, lng), -1.7851494503983558, 1.34e-14);
    CHECK_NEAR(*AGG::covar_samp(lat, lng), -1.8347369351316434, 1.34e-14);
    CHECK_NEAR(*AGG::corr(lat, lat), 1.0, 9.99e-15);
    CHECK_NEAR(*AGG::covar_samp(lng, lng), *AGG::variance(lng), 2 * 9.99e-15);   // each within 9.99e-15 of the exact variance
}

TEST(masked_moments_and_merged_shards) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const ChunkedArray& lat = df.column_by_name("lat").data();
    // the 12 cities north of 53 degrees: the mask is Column::filter's condition
    std::vector<ArrayRef> bits;
    for (auto& a : lat.chunks()) {
        std::vector<bool> b;
        for (double v : a->values_to_host<double>()) b.push_back(v > 53.0);
        bits.push_back(Array::from_bools(b));
    }
    const ChunkedArray mask = ChunkedArray::from_arrays(bits);
    const AGG::Moments north = AGG::moments(lat, &mask);
    CHECK_EQ(north.count(), (int64_t)12);
    CHECK_NEAR(*north.stat(RDF_STAT_VAR_SAMP), 2.798311962694546, 4.44e-15);
    CHECK_NEAR(*north.stat(RDF_STAT_SKEWNESS), 0.6266539972779798, 9.5e-15);
    CHECK_NEAR(*AGG::variance(lat.filter(mask)), *north.stat(RDF_STAT_VAR_SAMP), 8.88e-15);   // both within 4.44e-15 of the exact value
    // two slices of the column merge to the whole
    AGG::Moments a = AGG::moments(lat.slice(0, 20)), b = AGG::moments(lat.slice(20));
    CHECK_EQ(a.count() + b.count(), (int64_t)37);
    a.merge(b);
    CHECK_EQ(a.count(), (int64_t)37);
    CHECK_NEAR(*a.stat(RDF_STAT_VAR_SAMP), 3.6793042009666967, 9.99e-15);
    CHECK_NEAR(*a.stat(RDF_STAT_KURTOSIS), 0.830770544609576, 4.6e-14);
}

TEST(absent_statistics_and_refusals) {
    const ChunkedArray one = ChunkedArray::from_arrays({Array::from_vec<double>({2.5})});
    CHECK(!AGG::variance(one).has_value());
    CHECK(!AGG::skewness(one).has_value());
    CHECK_EQ(*AGG::var_pop(one), 0.0);
    const ChunkedArray flat = ChunkedArray::from_arrays({Array::from_vec<int64_t>({7, 7, 7, 7})});
    CHECK_EQ(*AGG::variance(flat), 0.0);
    CHECK(!AGG::kurtosis(flat).has_value());
    CHECK(!AGG::corr(flat, flat).has_value());
    const std::vector<bool> none = {false, false, false, false};
    const ChunkedArray nulls = ChunkedArray::from_arrays({Array::from_vec<int64_t>({1, 2, 3, 4}, &none)});
    CHECK(!AGG::var_pop(nulls).has_value());
    CHECK_EQ(AGG::moments(nulls).count(), (int64_t)0);
    const ChunkedArray flags = ChunkedArray::from_arrays({Array::from_bools({true, false})});
    CHECK_THROWS(AGG::variance(flags));
    const ChunkedArray two = ChunkedArray::from_arrays({Array::from_vec<double>({1.0, 3.0})});
    CHECK_THROWS(AGG::corr(two, flat));                       // chunk lengths differ
    CHECK_THROWS(AGG::variance(two, &two));                   // a mask that is not Boolean
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
