// Column::hist / Column::uniques in the C++ mirror (rdf_frame.hpp -> rdf_hist / rdf_uniques / rdf_utf8_uniques), run on the
// device: the two #[test]s of src/table.rs that read uk_cities_with_headers.csv (get_hist_column, :548-562;
// get_column_unique_values, :564-574) restated, plus the Utf8 column and a small column with repeats and NULLs.
#include <algorithm>
#include <cmath>
#include <set>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

TEST(get_hist_column) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const Column& lng = df.column(2);
    const Histogram h = lng.hist(10, true);
    CHECK_EQ(h.buckets().size(), (size_t)10);                        // the reference's assertion
    // the pinned semantics: numpy.histogram(lng, bins = 10)
    const uint64_t want[10] = {1, 1, 0, 2, 2, 4, 8, 8, 3, 8};
    uint64_t total = 0;
    for (size_t b = 0; b < 10; ++b) {
        CHECK_EQ(h.buckets()[b].count(), want[b]);
        total += h.buckets()[b].count();
        if (b) CHECK_EQ(h.buckets()[b].start(), h.buckets()[b - 1].end());
        CHECK_EQ(h.buckets()[b].density(), (double)want[b] / 37.0);
    }
    CHECK_EQ(total, (uint64_t)37);
    CHECK_EQ(h.num_samples(), (uint64_t)37);
    CHECK_EQ(h.buckets().front().start(), -7.318268);
    CHECK_EQ(h.buckets().back().end(), 0.573453);
    CHECK_EQ(h.buckets()[1].start(), -7.318268 + 1.0 * ((0.573453 - -7.318268) / 10.0));
    const Histogram plain = lng.hist(10, false);
    CHECK(!plain.has_density());
    CHECK_EQ(plain.buckets()[9].count(), (uint64_t)8);
    // one bucket takes every row; a text column has no histogram
    CHECK_EQ(lng.hist(1, false).buckets()[0].count(), (uint64_t)37);
    CHECK_THROWS(df.column(0).hist(10, false));
}

TEST(get_column_unique_values) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const GenericVector lat = df.column(1).uniques();
    CHECK_EQ(lat.kind, GenericVector::F);
    CHECK_EQ(lat.len(), (size_t)37);                                 // the reference's assertion
    std::vector<double> got = lat.f, all;
    for (auto& a : df.column(1).data().chunks()) { auto v = a->values_to_host<double>(); all.insert(all.end(), v.begin(), v.end()); }
    std::sort(got.begin(), got.end());
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    CHECK(got == all);
}

TEST(unique_city_names) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const GenericVector city = df.column(0).uniques();
    CHECK_EQ(city.kind, GenericVector::S);
    CHECK_EQ(city.len(), (size_t)37);
    std::set<std::string> want;
    for (auto& a : df.column(0).data().chunks())
        for (int64_t r = 0; r < a->length; ++r) want.insert((*a->strings)[(size_t)(a->offset + r)]);
    CHECK(std::set<std::string>(city.s.begin(), city.s.end()) == want);
    CHECK_EQ(want.size(), (size_t)37);
}

TEST(uniques_with_repeats_and_nulls) {
    const std::vector<bool> valid = {true, true, false, true, true, false, true, true};
    Column ints = Column::from_arrays({Array::from_vec<int64_t>({5, -1, 77, 5, 9, 78, -1, 5}, &valid), Array::from_vec<int64_t>({9, 9, 1000})},
                                      Field{"i", DataType::Int64, true});
    GenericVector g = ints.uniques();
    CHECK_EQ(g.kind, GenericVector::I);
    std::sort(g.i.begin(), g.i.end());
    CHECK(g.i == (std::vector<int64_t>{-1, 5, 9, 1000}));             // 77 and 78 only occur in NULL rows
    Column dbl = Column::from_arrays({Array::from_vec<double>({0.0, -0.0, 1.5, NAN, 1.5, -NAN, 0.0})}, Field{"d", DataType::Float64, false});
    GenericVector d = dbl.uniques();
    CHECK_EQ(d.len(), (size_t)3);                                    // one zero, 1.5, one NaN
    int nans = 0, zeros = 0;
    for (double x : d.f) { nans += std::isnan(x); zeros += x == 0.0 && !std::signbit(x); }
    CHECK_EQ(nans, 1);
    CHECK_EQ(zeros, 1);
    const Histogram h = ints.hist(4, true);                          // NULL rows are not counted
    CHECK_EQ(h.num_samples(), (uint64_t)9);
    CHECK_EQ(h.buckets()[0].count(), (uint64_t)8);
    CHECK_EQ(h.buckets()[3].count(), (uint64_t)1);
    CHECK_EQ(h.buckets()[0].start(), -1.0);
    CHECK_EQ(h.buckets()[3].end(), 1000.0);
    Column text = Column::from_arrays({Array::from_strings({"b", "a", "", "b", "a\0"}), Array::from_strings({"", "c"})}, Field{"t", DataType::Utf8, false});
    GenericVector t = text.uniques();
    std::sort(t.s.begin(), t.s.end());
    CHECK(t.s == (std::vector<std::string>{"", "a", "b", "c"}));
    Column flags = Column::from_arrays({Array::from_bools({true, false})}, Field{"f", DataType::Boolean, false});
    CHECK_THROWS(flags.uniques());
    CHECK_THROWS(flags.hist(2, false));
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
