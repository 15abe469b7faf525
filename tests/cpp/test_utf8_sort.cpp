// DataFrame::sort by a Utf8 column in the C++ mirror (rdf_frame.hpp -> rdf_lexsort_to_indices), run on the device: the
// reference's own dataset sorted by its text column, alone and with a numeric tie-breaker, and through a LazyFrame plan.
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

static std::vector<std::string> strings_of(const Column& c) {
    std::vector<std::string> out;
    for (auto& a : c.data().chunks())
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
static std::vector<double> doubles_of(const Column& c) {
    std::vector<double> out;
    for (auto& a : c.data().chunks()) {
        auto v = a->values_to_host<double>();
        out.insert(out.end(), v.begin(), v.begin() + a->length);
    }
    return out;
}

struct Rows { std::vector<std::string> city; std::vector<double> lat, lng; };
static Rows rows_of(const DataFrame& df) {
    return Rows{strings_of(df.column_by_name("city")), doubles_of(df.column_by_name("lat")), doubles_of(df.column_by_name("lng"))};
}
// the expected order: std::string compares as unsigned bytes, stable_sort keeps ties in row order
static std::vector<size_t> order_by_city(const Rows& r, bool descending) {
    std::vector<size_t> o(r.city.size());
    std::iota(o.begin(), o.end(), 0);
    std::stable_sort(o.begin(), o.end(), [&](size_t a, size_t b) { return descending ? r.city[b] < r.city[a] : r.city[a] < r.city[b]; });
    return o;
}
static void check_rows(const DataFrame& got, const Rows& in, const std::vector<size_t>& o) {
    const Rows g = rows_of(got);
    CHECK_EQ(g.city.size(), o.size());
    for (size_t i = 0; i < o.size(); ++i) {
        CHECK_EQ(g.city[i], in.city[o[i]]);
        CHECK_EQ(g.lat[i], in.lat[o[i]]);
        CHECK_EQ(g.lng[i], in.lng[o[i]]);
    }
}

TEST(test_sort_uk_cities_by_city) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const Rows in = rows_of(df);
    CHECK(in.city.size() > 30);
    DataFrame asc = df.sort({{"city"}});
    check_rows(asc, in, order_by_city(in, false));
    const Rows a = rows_of(asc);
    CHECK_EQ(a.city.front(), *std::min_element(in.city.begin(), in.city.end()));
    CHECK_EQ(a.city.back(), *std::max_element(in.city.begin(), in.city.end()));
    DataFrame desc = df.sort({{"city", true}});
    check_rows(desc, in, order_by_city(in, true));
    CHECK_EQ(rows_of(desc).city.front(), a.city.back());
}

TEST(test_sort_by_city_then_lat) {
    DataFrame df = DataFrame::from_csv(g_csv);
    const Rows in = rows_of(df);
    // criterion 0 text, criterion 1 numeric (descending): the order std::stable_sort gives for the same pair
    std::vector<size_t> o(in.city.size());
    std::iota(o.begin(), o.end(), 0);
    std::stable_sort(o.begin(), o.end(), [&](size_t a, size_t b) {
        if (in.city[a] != in.city[b]) return in.city[a] < in.city[b];
        return in.lat[a] > in.lat[b];
    });
    check_rows(df.sort({{"city"}, {"lat", true}}), in, o);
    // the same through a LazyFrame plan (Transformation::Sort)
    DataFrame lz = LazyFrame::read(df).sort({"city", "lat"}, {false, true}).evaluate();
    check_rows(lz, in, o);
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
