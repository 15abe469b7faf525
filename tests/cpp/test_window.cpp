// DataFrame::with_window in the C++ mirror (rdf_frame.hpp -> rdf_window), run on the device over uk_cities_with_headers.csv:
// rank of `lat` within a text partition column (the city's initial), lag / lead of the city name, ntile and row_number ordered
// by the text column.  The expected vectors were computed by tests/window_ref.py over the same file.
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
static std::vector<bool> valid_of(const Column& c) {
    std::vector<bool> out;
    for (auto& a : c.data().chunks()) { const auto v = a->valid_to_host(); out.insert(out.end(), v.begin(), v.end()); }
    return out;
}
template <class T> static std::vector<T> values_of(const Column& c) {
    std::vector<T> out;
    for (auto& a : c.data().chunks()) { const auto v = a->values_to_host<T>(); out.insert(out.end(), v.begin(), v.end()); }
    return out;
}

// the frame with a text partition column: the first letter of the city, chunked like the frame
static DataFrame cities() {
    DataFrame df = DataFrame::from_csv(g_csv);
    std::vector<ArrayRef> chunks;
    for (auto& a : df.column(0).data().chunks()) {
        std::vector<std::string> ini;
        for (int64_t r = 0; r < a->length; ++r) ini.push_back((*a->strings)[(size_t)(a->offset + r)].substr(0, 1));
        chunks.push_back(Array::from_strings(std::move(ini)));
    }
    return df.with_column("initial", Column::from_arrays(chunks, Field{"initial", DataType::Utf8, false}));
}

TEST(rank_of_lat_within_a_text_partition) {
    const DataFrame df = cities();
    CHECK_EQ(df.num_rows(), (int64_t)37);
    WindowSpec spec;
    spec.partition_by({"initial"}).order_by({DataFrame::SortCriteria{"lat", true, false}});
    const std::vector<int64_t> want = {1, 1, 3, 2, 2, 1, 3, 5, 1, 1, 1, 2, 2, 1, 4, 1, 1, 6, 3, 1, 1, 4, 1, 2, 3, 2, 3, 3, 1, 1, 2, 2, 1, 2, 1, 1, 1};
    const DataFrame r = df.with_window("rank", spec, WindowFunction::Rank);
    CHECK_EQ(r.num_columns(), df.num_columns() + 1);
    CHECK_EQ(r.column_by_name("rank").data().num_chunks(), df.num_chunks());
    CHECK(values_of<int64_t>(r.column_by_name("rank")) == want);
    CHECK(values_of<int64_t>(df.with_window("d", spec, WindowFunction::DenseRank).column_by_name("d")) == want);   // every lat is distinct
    const std::vector<double> cd = values_of<double>(df.with_window("c", spec, WindowFunction::CumeDist).column_by_name("c"));
    CHECK_EQ(cd[0], 0.5);
    CHECK_EQ(cd[1], 1.0 / 6.0);
    CHECK_EQ(cd[7], 5.0 / 6.0);
    CHECK_EQ(cd[26], 0.75);
    CHECK_EQ(cd[36], 1.0);
}

TEST(lag_and_lead_of_the_city_name) {
    const DataFrame df = cities();
    const std::vector<std::string> city = strings_of(df.column(0));
    WindowSpec spec;
    spec.partition_by({"initial"}).order_by({DataFrame::SortCriteria{"lat", false, false}});
    const int lag[37] = {4, 11, 14, 27, -1, -1, -1, 17, -1, -1, -1, 2, 24, 23, 7, 3, 31, -1, -1, 30, 33, -1, -1, -1, -1, 26, 21, -1, 25, -1, 18, 6, -1, -1, 12, -1, -1};
    const int lead2[37] = {-1, -1, 1, -1, -1, -1, 16, 2, -1, -1, -1, -1, -1, -1, 11, -1, -1, 14, 19, -1, -1, 25, -1, -1, 34, -1, 28, 15, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    const DataFrame a = df.with_window("prev", spec, WindowFunction::Lag, 1, "city");
    const DataFrame b = a.with_window("next2", spec, WindowFunction::Lead, 2, "city");
    CHECK(b.column_by_name("prev").data_type() == DataType::Utf8);
    const std::vector<std::string> prev = strings_of(b.column_by_name("prev")), next2 = strings_of(b.column_by_name("next2"));
    const std::vector<bool> pv = valid_of(b.column_by_name("prev")), nv = valid_of(b.column_by_name("next2"));
    for (int i = 0; i < 37; ++i) {
        CHECK_EQ((bool)pv[(size_t)i], lag[i] >= 0);
        CHECK_EQ((bool)nv[(size_t)i], lead2[i] >= 0);
        if (lag[i] >= 0) CHECK_EQ(prev[(size_t)i], city[(size_t)lag[i]]);
        if (lead2[i] >= 0) CHECK_EQ(next2[(size_t)i], city[(size_t)lead2[i]]);
    }
    // a numeric value column through the same indices: lag(lat) is the lat of the city lag(city) names
    const DataFrame c = df.with_window("plat", spec, WindowFunction::Lag, 1, "lat");
    const std::vector<double> lat = values_of<double>(df.column(1)), plat = values_of<double>(c.column_by_name("plat"));
    const std::vector<bool> lv = valid_of(c.column_by_name("plat"));
    for (int i = 0; i < 37; ++i) {
        CHECK_EQ((bool)lv[(size_t)i], lag[i] >= 0);
        if (lag[i] >= 0) CHECK_EQ(plat[(size_t)i], lat[(size_t)lag[i]]);
    }
    CHECK_THROWS(df.with_window("x", spec, WindowFunction::Lag, 1));          // no value column
    CHECK_THROWS(df.with_window("x", spec, WindowFunction::Ntile, 0));        // no buckets
}

TEST(ntile_and_row_number_ordered_by_the_text_column) {
    const DataFrame df = cities();
    WindowSpec spec;
    spec.order_by({DataFrame::SortCriteria{"city", false, false}});
    const std::vector<int64_t> nt = {2, 4, 4, 1, 2, 3, 3, 4, 2, 3, 3, 4, 2, 1, 4, 1, 3, 3, 4, 4, 3, 1, 1, 1, 2, 1, 1, 1, 1, 4, 4, 3, 2, 3, 2, 2, 2};
    const std::vector<int64_t> rn = {12, 30, 29, 7, 11, 24, 21, 33, 14, 23, 27, 31, 15, 1, 32, 8, 22, 28, 35, 36, 26, 6, 10, 2, 16, 4, 3, 9, 5, 34, 37, 20, 19, 25, 17, 13, 18};
    CHECK(values_of<int64_t>(df.with_window("t", spec, WindowFunction::Ntile, 4).column_by_name("t")) == nt);
    CHECK(values_of<int64_t>(df.with_window("n", spec, WindowFunction::RowNumber).column_by_name("n")) == rn);
    // no keys at all: row order
    const std::vector<int64_t> plain = values_of<int64_t>(df.with_window("n", WindowSpec(), WindowFunction::RowNumber).column_by_name("n"));
    for (int i = 0; i < 37; ++i) CHECK_EQ(plain[(size_t)i], (int64_t)i + 1);
    const std::vector<double> pr = values_of<double>(df.with_window("p", WindowSpec(), WindowFunction::PercentRank).column_by_name("p"));
    for (int i = 0; i < 37; ++i) CHECK_EQ(pr[(size_t)i], 0.0);                 // every row a peer of every other
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
