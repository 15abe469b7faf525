// WindowSpec::rows_between / range_between and DataFrame::with_window_agg in the C++ mirror (rdf_frame.hpp -> rdf_window_agg), run
// on the device over uk_cities_with_headers.csv: cities partitioned by their initial and ordered by `lat`, aggregates of the row
// number `row` (Int64) and of `lat` (Float64) over ROWS and RANGE frames, first / last value of the city name.  The expected
// vectors were computed by tests/window_frame_ref.py over the same file.
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

// the frame with a text partition column (the first letter of the city) and the row number, chunked like the frame
static DataFrame cities() {
    DataFrame df = DataFrame::from_csv(g_csv);
    std::vector<ArrayRef> ini_chunks, row_chunks;
    int64_t at = 0;
    for (auto& a : df.column(0).data().chunks()) {
        std::vector<std::string> ini;
        std::vector<int64_t> row;
        for (int64_t r = 0; r < a->length; ++r) { ini.push_back((*a->strings)[(size_t)(a->offset + r)].substr(0, 1)); row.push_back(at++); }
        ini_chunks.push_back(Array::from_strings(std::move(ini)));
        row_chunks.push_back(Array::from_vec<int64_t>(row));
    }
    return df.with_column("initial", Column::from_arrays(ini_chunks, Field{"initial", DataType::Utf8, false}))
        .with_column("row", Column::from_arrays(row_chunks, Field{"row", DataType::Int64, false}));
}

static WindowSpec by_initial_and_lat() {
    WindowSpec spec;
    spec.partition_by({"initial"}).order_by({DataFrame::SortCriteria{"lat", false, false}});
    return spec;
}

TEST(sum_avg_and_count_over_rows_frames) {
    const DataFrame df = cities();
    CHECK_EQ(df.num_rows(), (int64_t)37);
    WindowSpec spec = by_initial_and_lat();
    spec.rows_between(-1, WindowSpec::current_row);
    const std::vector<int64_t> sum_prev = {4, 12, 16, 30, 4, 5, 6, 24, 8, 9, 10, 13, 36, 36, 21, 18, 47, 17, 18, 49, 53, 21, 22, 23, 24, 51, 47, 27, 53, 29, 48, 37, 32, 33, 46, 35, 36};
    const std::vector<double> avg_prev = {2.0, 6.0, 8.0, 15.0, 4.0, 5.0, 6.0, 12.0, 8.0, 9.0, 10.0, 6.5, 18.0, 18.0, 10.5, 9.0, 23.5, 17.0, 18.0, 24.5, 26.5, 21.0, 22.0, 23.0, 24.0, 25.5, 23.5, 27.0, 26.5, 29.0, 24.0, 18.5, 32.0, 33.0, 23.0, 35.0, 36.0};
    const DataFrame r = df.with_window_agg("s", spec, WindowAggregate::Sum, "row");
    CHECK_EQ(r.num_columns(), df.num_columns() + 1);
    CHECK_EQ(r.column_by_name("s").data().num_chunks(), df.num_chunks());
    CHECK(r.column_by_name("s").data_type() == DataType::Int64);
    CHECK(values_of<int64_t>(r.column_by_name("s")) == sum_prev);
    CHECK(values_of<double>(df.with_window_agg("a", spec, WindowAggregate::Avg, "row").column_by_name("a")) == avg_prev);
    // 1 FOLLOWING .. 2 FOLLOWING: the frame slides off the partition's end; COUNT(*) is 0 there, never NULL
    spec.rows_between(1, 2);
    const std::vector<int64_t> cnt = {0, 0, 2, 1, 1, 0, 2, 2, 0, 0, 0, 1, 1, 0, 2, 0, 0, 2, 2, 0, 0, 2, 0, 1, 2, 1, 2, 2, 0, 0, 1, 1, 0, 1, 0, 0, 0};
    CHECK(values_of<int64_t>(df.with_window_agg("c", spec, WindowAggregate::Count).column_by_name("c")) == cnt);
    const DataFrame e = df.with_window_agg("s", spec, WindowAggregate::Sum, "row");     // SUM over an empty frame is NULL
    const std::vector<bool> sv = valid_of(e.column_by_name("s"));
    for (int i = 0; i < 37; ++i) CHECK_EQ((bool)sv[(size_t)i], cnt[(size_t)i] > 0);
    // the whole partition
    spec.rows_between(WindowSpec::unbounded_preceding, WindowSpec::unbounded_following);
    const std::vector<int64_t> tot = {4, 52, 52, 45, 4, 5, 53, 52, 8, 9, 10, 52, 70, 36, 52, 45, 53, 52, 67, 67, 53, 100, 22, 36, 70, 100, 100, 45, 100, 29, 67, 53, 32, 53, 70, 35, 36};
    CHECK(values_of<int64_t>(df.with_window_agg("t", spec, WindowAggregate::Sum, "row").column_by_name("t")) == tot);
}

TEST(min_and_max_of_a_float64_column_and_the_default_frame) {
    const DataFrame df = cities();
    const std::vector<double> lat = values_of<double>(df.column(1));
    WindowSpec spec = by_initial_and_lat();
    spec.rows_between(-1, 1);
    const int mx[37] = {0, 1, 11, 15, 0, 5, 31, 14, 8, 9, 10, 1, 34, 13, 2, 15, 16, 7, 30, 19, 20, 26, 22, 13, 12, 28, 25, 3, 28, 29, 19, 16, 32, 20, 34, 35, 36};
    const std::vector<double> got_mx = values_of<double>(df.with_window_agg("m", spec, WindowAggregate::Max, "lat").column_by_name("m"));
    for (int i = 0; i < 37; ++i) CHECK_EQ(got_mx[(size_t)i], lat[(size_t)mx[i]]);
    // no frame set: RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW, the running minimum
    const int mn[37] = {4, 17, 17, 27, 4, 5, 6, 17, 8, 9, 10, 17, 24, 23, 17, 27, 6, 17, 18, 18, 33, 21, 22, 23, 24, 21, 21, 27, 21, 29, 18, 6, 32, 33, 24, 35, 36};
    const WindowSpec dflt = by_initial_and_lat();
    const std::vector<double> got_mn = values_of<double>(df.with_window_agg("m", dflt, WindowAggregate::Min, "lat").column_by_name("m"));
    for (int i = 0; i < 37; ++i) CHECK_EQ(got_mn[(size_t)i], lat[(size_t)mn[i]]);
    // ... and without order keys every row of the partition is a peer: the default frame is the whole partition
    WindowSpec unordered;
    unordered.partition_by({"initial"});
    const std::vector<int64_t> cp = {2, 6, 6, 3, 2, 1, 3, 6, 1, 1, 1, 6, 3, 2, 6, 3, 3, 6, 3, 3, 2, 4, 1, 2, 3, 4, 4, 3, 4, 1, 3, 3, 1, 2, 3, 1, 1};
    CHECK(values_of<int64_t>(df.with_window_agg("c", unordered, WindowAggregate::Count, "row").column_by_name("c")) == cp);
    // with_window ignores the frame of a spec
    WindowSpec framed = by_initial_and_lat();
    framed.rows_between(-1, 1);
    CHECK(values_of<int64_t>(df.with_window("r", framed, WindowFunction::Rank).column_by_name("r")) ==
          values_of<int64_t>(df.with_window("r", by_initial_and_lat(), WindowFunction::Rank).column_by_name("r")));
}

TEST(first_and_last_value_of_the_city_name_and_what_is_refused) {
    const DataFrame df = cities();
    const std::vector<std::string> city = strings_of(df.column(0));
    WindowSpec spec = by_initial_and_lat();
    spec.rows_between(1, 1);                                                   // lead(city, 1) spelled as a frame
    const int first[37] = {-1, -1, 11, 15, 0, -1, 31, 14, -1, -1, -1, 1, 34, -1, 2, -1, -1, 7, 30, -1, -1, 26, -1, 13, 12, 28, 25, 3, -1, -1, 19, 16, -1, 20, -1, -1, -1};
    const DataFrame a = df.with_window_agg("next", spec, WindowAggregate::FirstValue, "city");
    CHECK(a.column_by_name("next").data_type() == DataType::Utf8);
    const std::vector<std::string> next = strings_of(a.column_by_name("next"));
    const std::vector<bool> nv = valid_of(a.column_by_name("next"));
    spec.rows_between(WindowSpec::unbounded_preceding, WindowSpec::unbounded_following);
    const int last[37] = {0, 1, 1, 15, 0, 5, 16, 1, 8, 9, 10, 1, 34, 13, 1, 15, 16, 1, 19, 19, 20, 28, 22, 13, 34, 28, 28, 15, 28, 29, 19, 16, 32, 20, 34, 35, 36};
    const std::vector<std::string> north = strings_of(df.with_window_agg("north", spec, WindowAggregate::LastValue, "city").column_by_name("north"));
    for (int i = 0; i < 37; ++i) {
        CHECK_EQ((bool)nv[(size_t)i], first[i] >= 0);
        if (first[i] >= 0) CHECK_EQ(next[(size_t)i], city[(size_t)first[i]]);
        CHECK_EQ(north[(size_t)i], city[(size_t)last[i]]);
    }
    CHECK_THROWS(df.with_window_agg("x", spec, WindowAggregate::Sum));          // no value column
    CHECK_THROWS(df.with_window_agg("x", spec, WindowAggregate::Sum, "city"));  // a text column has no sum
    WindowSpec bad = by_initial_and_lat();
    bad.rows_between(1, -1);
    CHECK_THROWS(df.with_window_agg("x", bad, WindowAggregate::Sum, "row"));    // the frame starts after its end
    bad.range_between(-1, 0);
    CHECK_THROWS(df.with_window_agg("x", bad, WindowAggregate::Sum, "row"));    // range offsets are not built
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
