// WindowSpec::range_by and DataFrame::with_window_agg in the C++ mirror (rdf_frame.hpp -> rdf_window_range_agg), run on the device
// over uk_cities_with_headers.csv: cities partitioned by their initial and ordered by `lat` (Float64), frames of half a degree
// around the row, ahead of it and behind it, both directions; and the row number `row` (Int64) as the order key of a frame of
// three rows back.  The expected vectors were computed by tests/window_range_ref.py over the same file.
#include <limits>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

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
static std::vector<std::string> strings_of(const Column& c) {
    std::vector<std::string> out;
    for (auto& a : c.data().chunks())
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
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

static WindowSpec by_initial_and_lat(bool descending = false) {
    WindowSpec spec;
    spec.partition_by({"initial"}).order_by({DataFrame::SortCriteria{"lat", descending, false}});
    return spec;
}

TEST(cities_within_half_a_degree_of_latitude) {
    const DataFrame df = cities();
    CHECK_EQ(df.num_rows(), (int64_t)37);
    WindowSpec spec = by_initial_and_lat();
    spec.range_by(-0.5, 0.5);
    const std::vector<int64_t> sum_half = {0, 12, 13, 30, 4, 5, 6, 38, 8, 9, 10, 14, 46, 13, 21, 15, 16, 24, 48, 19, 20, 21, 22, 23, 24, 25, 26, 30, 28, 29, 48, 31, 32, 33, 46, 35, 36};
    const std::vector<int64_t> cnt_half = {1, 2, 2, 2, 1, 1, 1, 3, 1, 1, 1, 3, 2, 1, 2, 1, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1, 2, 1, 1, 1, 2, 1, 1};
    const std::vector<double> avg_half = {0.0, 6.0, 6.5, 15.0, 4.0, 5.0, 6.0, 12.666666666666666, 8.0, 9.0, 10.0, 4.666666666666667, 23.0, 13.0, 10.5, 15.0, 16.0, 12.0, 24.0, 19.0, 20.0, 21.0, 22.0, 23.0, 24.0, 25.0, 26.0, 15.0, 28.0, 29.0, 24.0, 31.0, 32.0, 33.0, 23.0, 35.0, 36.0};
    const DataFrame r = df.with_window_agg("s", spec, WindowAggregate::Sum, "row");
    CHECK_EQ(r.num_columns(), df.num_columns() + 1);
    CHECK_EQ(r.column_by_name("s").data().num_chunks(), df.num_chunks());
    CHECK(r.column_by_name("s").data_type() == DataType::Int64);
    CHECK(values_of<int64_t>(r.column_by_name("s")) == sum_half);
    CHECK(values_of<int64_t>(df.with_window_agg("c", spec, WindowAggregate::Count).column_by_name("c")) == cnt_half);
    CHECK(values_of<double>(df.with_window_agg("a", spec, WindowAggregate::Avg, "row").column_by_name("a")) == avg_half);
    // descending, half a degree PRECEDING is half a degree further north
    WindowSpec north = by_initial_and_lat(true);
    north.range_by(-0.5, 0.0);
    const std::vector<int64_t> sum_desc = {0, 1, 13, 3, 4, 5, 6, 21, 8, 9, 10, 12, 46, 13, 14, 15, 16, 24, 48, 19, 20, 21, 22, 23, 24, 25, 26, 30, 28, 29, 30, 31, 32, 33, 34, 35, 36};
    CHECK(values_of<int64_t>(df.with_window_agg("s", north, WindowAggregate::Sum, "row").column_by_name("s")) == sum_desc);
}

TEST(frames_ahead_of_the_row_are_often_empty) {
    const DataFrame df = cities();
    WindowSpec spec = by_initial_and_lat();
    spec.range_by(0.25, 1.0);                                                   // 0.25 FOLLOWING .. 1 FOLLOWING
    const std::vector<int64_t> cnt = {0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 2, 0, 0, 2, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const std::vector<int64_t> sum = {0, 0, 1, 0, 0, 0, 0, 2, 0, 0, 0, 1, 34, 0, 13, 0, 0, 21, 0, 0, 0, 26, 0, 0, 12, 0, 25, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(values_of<int64_t>(df.with_window_agg("c", spec, WindowAggregate::Count).column_by_name("c")) == cnt);   // COUNT(*) is 0, never NULL
    const DataFrame e = df.with_window_agg("s", spec, WindowAggregate::Sum, "row");                                   // SUM over an empty frame is NULL
    const std::vector<bool> sv = valid_of(e.column_by_name("s"));
    const std::vector<int64_t> got = values_of<int64_t>(e.column_by_name("s"));
    for (int i = 0; i < 37; ++i) {
        CHECK_EQ((bool)sv[(size_t)i], cnt[(size_t)i] > 0);
        if (cnt[(size_t)i] > 0) CHECK_EQ(got[(size_t)i], sum[(size_t)i]);
    }
    // 1 PRECEDING .. 0.1 PRECEDING: the southernmost city of the frame, by name
    const std::vector<std::string> city = strings_of(df.column(0));
    spec.range_by(-1.0, -0.1);
    const int first[37] = {-1, 2, 7, -1, -1, -1, -1, 17, -1, -1, -1, 14, 24, -1, 17, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 26, 21, -1, -1, -1, 18, -1, -1, -1, 12, -1, -1};
    const DataFrame f = df.with_window_agg("south", spec, WindowAggregate::FirstValue, "city");
    CHECK(f.column_by_name("south").data_type() == DataType::Utf8);
    const std::vector<std::string> south = strings_of(f.column_by_name("south"));
    const std::vector<bool> fv = valid_of(f.column_by_name("south"));
    for (int i = 0; i < 37; ++i) {
        CHECK_EQ((bool)fv[(size_t)i], first[i] >= 0);
        if (first[i] >= 0) CHECK_EQ(south[(size_t)i], city[(size_t)first[i]]);
    }
}

TEST(max_with_one_unbounded_side_and_an_integer_order_key) {
    const DataFrame df = cities();
    const std::vector<double> lat = values_of<double>(df.column(1));
    WindowSpec spec = by_initial_and_lat();
    spec.range_by(-std::numeric_limits<double>::infinity(), 0.5);               // UNBOUNDED PRECEDING .. 0.5 FOLLOWING: the running maximum, half a degree ahead
    const int mx[37] = {0, 1, 11, 3, 4, 5, 6, 14, 8, 9, 10, 1, 34, 13, 14, 15, 16, 7, 30, 19, 20, 21, 22, 23, 24, 25, 26, 3, 28, 29, 30, 31, 32, 33, 34, 35, 36};
    const std::vector<double> got_mx = values_of<double>(df.with_window_agg("m", spec, WindowAggregate::Max, "lat").column_by_name("m"));
    for (int i = 0; i < 37; ++i) CHECK_EQ(got_mx[(size_t)i], lat[(size_t)mx[i]]);
    spec.range_by(WindowSpec::unbounded_preceding, 0);                          // the integer form names the sentinels, but a Float64 key takes doubles
    CHECK_THROWS(df.with_window_agg("m", spec, WindowAggregate::Max, "lat"));
    WindowSpec upto;                                                            // the whole column ordered by the Int64 row number
    upto.order_by({DataFrame::SortCriteria{"row", false, false}});
    upto.range_by(-3, WindowSpec::unbounded_following);
    const std::vector<double> mn = values_of<double>(df.with_window_agg("m", upto, WindowAggregate::Min, "lat").column_by_name("m"));
    for (int i = 0; i < 37; ++i) CHECK_EQ(mn[(size_t)i], lat[33]);              // the southernmost city is row 33: inside every frame that runs to the end
    upto.range_by(-3, 0);
    const std::vector<int64_t> cnt = {1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
    CHECK(values_of<int64_t>(df.with_window_agg("c", upto, WindowAggregate::Count, "lat").column_by_name("c")) == cnt);
    CHECK_THROWS(df.with_window_agg("m", upto, WindowAggregate::Max, "lat"));   // min / max over a range frame bounded on both sides is not built
}

TEST(what_range_by_refuses) {
    const DataFrame df = cities();
    WindowSpec text;
    text.order_by({DataFrame::SortCriteria{"city", false, false}});
    text.range_by(-1, 0);
    CHECK_THROWS(df.with_window_agg("x", text, WindowAggregate::Count));        // a text order column has no distances
    text.range_by(-1.0, 0.0);
    CHECK_THROWS(df.with_window_agg("x", text, WindowAggregate::Count));
    WindowSpec two = by_initial_and_lat();
    two.order_by({DataFrame::SortCriteria{"lat", false, false}, DataFrame::SortCriteria{"row", false, false}});
    two.range_by(-0.5, 0.5);
    CHECK_THROWS(df.with_window_agg("x", two, WindowAggregate::Count));         // exactly one order column
    WindowSpec none;
    none.partition_by({"initial"});
    none.range_by(-1, 1);
    CHECK_THROWS(df.with_window_agg("x", none, WindowAggregate::Count));
    WindowSpec wrong = by_initial_and_lat();
    wrong.range_by(-1, 1);                                                      // integer offsets over a Float64 column
    CHECK_THROWS(df.with_window_agg("x", wrong, WindowAggregate::Count));
    WindowSpec rows;
    rows.order_by({DataFrame::SortCriteria{"row", false, false}});
    rows.range_by(-0.5, 0.5);                                                   // double offsets over an Int64 column
    CHECK_THROWS(df.with_window_agg("x", rows, WindowAggregate::Count));
    rows.range_by(1, -1);                                                       // the frame starts after its end
    CHECK_THROWS(df.with_window_agg("x", rows, WindowAggregate::Count));
    rows.range_between(-1, 0);                                                  // range_between with offsets keeps throwing
    CHECK_THROWS(df.with_window_agg("x", rows, WindowAggregate::Count));
    rows.rows_between(-1, 0);                                                   // ... and a later rows_between replaces range_by
    const std::vector<int64_t> c = values_of<int64_t>(df.with_window_agg("c", rows, WindowAggregate::Count).column_by_name("c"));
    CHECK_EQ(c[0], (int64_t)1);
    CHECK_EQ(c[36], (int64_t)2);
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
