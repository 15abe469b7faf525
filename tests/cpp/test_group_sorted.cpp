// count_distinct / sum_distinct / first / last in the C++ mirror (rdf_frame.hpp -> rdf_groupby_sorted), run on the device:
// the four AggregateFunctions on small columns (empty and all-NULL included), and a GroupAggregate step that mixes Sum with
// CountDistinct / First / Last over an integer key with a NULL and over a Utf8 key, row for row against typed-in answers
// with the names and dtypes Dataset::try_aggregate plans.
#include <cmath>
#include <optional>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
namespace P = rdf::plan;
using AF = P::AggregateFunction;
using AGG = AggregateFunctions;

template <class T> static Column num(const std::string& name, const std::vector<T>& v, const std::vector<bool>* valid = nullptr) {
    return Column::from_arrays({Array::from_vec<T>(v, valid)}, Field{name, TypeOf<T>::value, true});
}
static Column text(const std::string& name, std::vector<std::string> rows, const std::vector<bool>* valid = nullptr) {
    auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(rows)));
    if (valid) {
        const auto bits = pack_bits(*valid);
        a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
        check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
        for (bool b : *valid) a->null_count += !b;
    }
    return Column::from_arrays({ArrayRef(a)}, Field{name, DataType::Utf8, true});
}
// one column as optional values, NULL rows as nullopt
template <class T> static std::vector<std::optional<T>> rows_of(const Column& c) {
    std::vector<std::optional<T>> out;
    for (auto& a : c.data().chunks()) {
        const auto v = a->values_to_host<T>();
        const auto ok = a->valid_to_host();
        for (size_t r = 0; r < v.size(); ++r) out.push_back(ok[r] ? std::optional<T>(v[r]) : std::nullopt);
    }
    return out;
}
static std::vector<std::optional<std::string>> strings_of(const Column& c) {
    std::vector<std::optional<std::string>> out;
    for (auto& a : c.data().chunks()) {
        const auto ok = a->valid_to_host();
        for (int64_t r = 0; r < a->length; ++r) out.push_back(ok[(size_t)r] ? std::optional<std::string>((*a->strings)[(size_t)(a->offset + r)]) : std::nullopt);
    }
    return out;
}
template <class T> using Opt = std::vector<std::optional<T>>;
static const std::nullopt_t N = std::nullopt;

TEST(whole_column_aggregates_of_numeric_columns) {
    const Column f = num<double>("f", {-0.0, 0.0, 1.5, 2.5, 1.5});
    CHECK_EQ(AGG::count_distinct(f), (int64_t)3);                       // rdf_uniques' route: -0.0 and +0.0 are one value
    CHECK_EQ(AGG::sum_distinct<double>(f), 4.0);
    const Column fn = num<double>("f", {1.0, std::nan(""), -std::nan(""), 1.0});
    CHECK_EQ(AGG::count_distinct(fn), (int64_t)2);
    CHECK(std::isnan(AGG::sum_distinct<double>(fn)));
    const std::vector<bool> valid{true, true, true, false};
    const Column i = num<int32_t>("i", {3, 3, -1, 7}, &valid);
    CHECK_EQ(AGG::count_distinct(i), (int64_t)2);                       // Int32: the sorted route
    CHECK_EQ(AGG::sum_distinct<int64_t>(i), (int64_t)2);
    CHECK(rows_of<int32_t>(*AGG::first(i)) == (Opt<int32_t>{3}));
    CHECK(rows_of<int32_t>(*AGG::last(i)) == (Opt<int32_t>{N}));        // the last row is NULL: SQL's last(x)
    CHECK(rows_of<int32_t>(*AGG::last(i, true)) == (Opt<int32_t>{-1}));
    CHECK(rows_of<int32_t>(*AGG::first(i, true)) == (Opt<int32_t>{3}));
    const Column u = num<uint64_t>("u", {~0ull, 2, ~0ull});
    CHECK_EQ(AGG::sum_distinct<uint64_t>(u), (uint64_t)1);              // wraps mod 2^64
    CHECK_THROWS(AGG::sum_distinct<double>(i));
    CHECK_THROWS(AGG::sum_distinct<int64_t>(f));
}

TEST(whole_column_aggregates_of_empty_and_all_null_columns) {
    const Column e = num<int64_t>("e", {});
    CHECK_EQ(AGG::count_distinct(e), (int64_t)0);
    CHECK_EQ(AGG::sum_distinct<int64_t>(e), (int64_t)0);
    CHECK(!AGG::first(e) && !AGG::last(e) && !AGG::first(e, true));
    const std::vector<bool> none{false, false, false};
    const Column n = num<int16_t>("n", {4, 5, 6}, &none);
    CHECK_EQ(AGG::count_distinct(n), (int64_t)0);
    CHECK_EQ(AGG::sum_distinct<int64_t>(n), (int64_t)0);
    CHECK(!AGG::first(n, true) && !AGG::last(n, true));
    CHECK(rows_of<int16_t>(*AGG::first(n)) == (Opt<int16_t>{N}));
    const Column nf = num<double>("nf", {4, 5, 6}, &none);
    CHECK_EQ(AGG::count_distinct(nf), (int64_t)0);
    CHECK_EQ(AGG::sum_distinct<double>(nf), 0.0);
}

TEST(whole_column_aggregates_of_a_utf8_column) {
    const std::vector<bool> valid{true, true, false, true, true};
    const Column s = text("s", {"b", "", "zz", "b", "a"}, &valid);
    CHECK_EQ(AGG::count_distinct(s), (int64_t)3);                       // "", "a", "b": the empty string is a value, NULL is not
    CHECK(strings_of(*AGG::first(s)) == (Opt<std::string>{std::string("b")}));
    CHECK(strings_of(*AGG::last(s)) == (Opt<std::string>{std::string("a")}));
    const std::vector<bool> tail{true, true, false};
    const Column t = text("t", {"x", "y", ""}, &tail);
    CHECK(strings_of(*AGG::last(t)) == (Opt<std::string>{N}));
    CHECK(strings_of(*AGG::last(t, true)) == (Opt<std::string>{std::string("y")}));
    CHECK_THROWS(AGG::sum_distinct<int64_t>(s));
    CHECK_EQ(AGG::count_distinct(text("z", {})), (int64_t)0);
}

//  row   0    1    2     3    4     5     6
//  k     2    1    NULL  2    1     NULL  2
//  v     5    7    9     5    NULL  9     6
//  w     5    7    9     5    8     9     6
//  s     b    a    ""    b    c     x     a
static DataFrame frame() {
    const std::vector<bool> kvalid{true, true, false, true, true, false, true}, vvalid{true, true, true, true, false, true, true};
    return DataFrame::from_columns({num<int64_t>("k", {2, 1, 0, 2, 1, 0, 2}, &kvalid), num<int64_t>("v", {5, 7, 9, 5, 8, 9, 6}, &vvalid),
                                    num<int64_t>("w", {5, 7, 9, 5, 8, 9, 6}), text("s", {"b", "a", "", "b", "c", "x", "a"})});
}

static void check_by_k(const DataFrame& g) {
    CHECK_EQ(g.num_columns(), (size_t)8);
    const char* names[] = {"k", "sum(v)", "count_distinct(v)", "count_distinct(s)", "first(v)", "first(s)", "last(v)", "last(s)"};
    const DataType types[] = {DataType::Int64, DataType::Int64, DataType::UInt32, DataType::UInt32, DataType::Int64, DataType::Utf8, DataType::Int64, DataType::Utf8};
    for (size_t c = 0; c < 8; ++c) { CHECK_EQ(g.column(c).name(), std::string(names[c])); CHECK(g.column(c).data_type() == types[c]); }
    CHECK(rows_of<int64_t>(g.column(0)) == (Opt<int64_t>{1, 2, N}));                      // ascending, the NULL group last
    CHECK(rows_of<int64_t>(g.column(1)) == (Opt<int64_t>{7, 16, 18}));
    CHECK(rows_of<uint32_t>(g.column(2)) == (Opt<uint32_t>{1, 2, 1}));
    CHECK(rows_of<uint32_t>(g.column(3)) == (Opt<uint32_t>{2, 2, 2}));
    CHECK(rows_of<int64_t>(g.column(4)) == (Opt<int64_t>{7, 5, 9}));
    CHECK(strings_of(g.column(5)) == (Opt<std::string>{std::string("a"), std::string("b"), std::string("")}));
    CHECK(rows_of<int64_t>(g.column(6)) == (Opt<int64_t>{N, 6, 9}));                      // row 4 is the last of k = 1 and its v is NULL
    CHECK(strings_of(g.column(7)) == (Opt<std::string>{std::string("c"), std::string("a"), std::string("x")}));
}

TEST(group_aggregate_over_an_integer_key_with_a_null) {
    const std::vector<P::Aggregation> aggs{{AF::Sum, {"v"}}, {AF::CountDistinct, {"v", "s"}}, {AF::First, {"v", "s"}}, {AF::Last, {"v", "s"}}};
    check_by_k(Evaluate::group_aggregate(frame(), {"k"}, aggs));
    check_by_k(LazyFrame::read(frame()).aggregate({"k"}, aggs).evaluate());                // the plan's GroupAggregate step
    // the sorted aggregations first: they then supply the key column
    const DataFrame g = Evaluate::group_aggregate(frame(), {"k"}, {{AF::Last, {"w"}}, {AF::Sum, {"w"}}});
    CHECK(rows_of<int64_t>(g.column(0)) == (Opt<int64_t>{1, 2, N}));
    CHECK(rows_of<int64_t>(g.column_by_name("last(w)")) == (Opt<int64_t>{8, 6, 9}));
    CHECK(rows_of<int64_t>(g.column_by_name("sum(w)")) == (Opt<int64_t>{15, 16, 18}));
}

TEST(group_aggregate_over_a_utf8_key) {
    const DataFrame g = Evaluate::group_aggregate(frame(), {"s"}, {{AF::Sum, {"w"}}, {AF::CountDistinct, {"w"}}, {AF::First, {"w", "k"}}, {AF::Last, {"w"}}});
    CHECK_EQ(g.num_columns(), (size_t)6);
    const char* names[] = {"s", "sum(w)", "count_distinct(w)", "first(w)", "first(k)", "last(w)"};
    for (size_t c = 0; c < 6; ++c) CHECK_EQ(g.column(c).name(), std::string(names[c]));
    CHECK(g.column(0).data_type() == DataType::Utf8 && g.column(2).data_type() == DataType::UInt32 && g.column(4).data_type() == DataType::Int64);
    CHECK(strings_of(g.column(0)) == (Opt<std::string>{std::string(""), std::string("a"), std::string("b"), std::string("c"), std::string("x")}));
    CHECK(rows_of<int64_t>(g.column(1)) == (Opt<int64_t>{9, 13, 10, 8, 9}));
    CHECK(rows_of<uint32_t>(g.column(2)) == (Opt<uint32_t>{1, 2, 1, 1, 1}));
    CHECK(rows_of<int64_t>(g.column(3)) == (Opt<int64_t>{9, 7, 5, 8, 9}));
    CHECK(rows_of<int64_t>(g.column(4)) == (Opt<int64_t>{N, 1, 2, 1, N}));
    CHECK(rows_of<int64_t>(g.column(5)) == (Opt<int64_t>{9, 6, 5, 8, 9}));
    // two keys, text and integer: (s, k) pairs in order, the NULL k last inside its s
    const DataFrame h = Evaluate::group_aggregate(frame(), {"s", "k"}, {{AF::Sum, {"w"}}, {AF::CountDistinct, {"w"}}, {AF::Last, {"s"}}});
    CHECK(strings_of(h.column(0)) == (Opt<std::string>{std::string(""), std::string("a"), std::string("a"), std::string("b"), std::string("c"), std::string("x")}));
    CHECK(rows_of<int64_t>(h.column(1)) == (Opt<int64_t>{N, 1, 2, 2, 1, N}));
    CHECK(rows_of<int64_t>(h.column_by_name("sum(w)")) == (Opt<int64_t>{9, 7, 6, 10, 8, 9}));   // the hash aggregation, row for row
    CHECK(rows_of<uint32_t>(h.column_by_name("count_distinct(w)")) == (Opt<uint32_t>{1, 1, 1, 1, 1, 1}));
    CHECK(strings_of(h.column_by_name("last(s)")) == strings_of(h.column(0)));
}

//  row   0    1    2    3    4    5    6
//  s     a    a    a    b    b    ""   a
//  k     NULL 2    1    NULL 1    3    NULL
//  w     1    2    4    8    16   32   64
TEST(hash_and_sorted_aggregations_line_up_over_two_keys_with_nulls) {
    const std::vector<bool> kvalid{false, true, true, false, true, true, false};
    const DataFrame f = DataFrame::from_columns({text("s", {"a", "a", "a", "b", "b", "", "a"}), num<int64_t>("k", {0, 2, 1, 0, 1, 3, 0}, &kvalid),
                                                 num<int64_t>("w", {1, 2, 4, 8, 16, 32, 64})});
    // a NULL k and other k inside one s: the NULL last inside its s, for the hash results and the sorted ones alike
    for (const bool hash_first : {true, false}) {
        const std::vector<P::Aggregation> aggs = hash_first ? std::vector<P::Aggregation>{{AF::Sum, {"w"}}, {AF::CountDistinct, {"w"}}, {AF::Last, {"w"}}}
                                                            : std::vector<P::Aggregation>{{AF::Last, {"w"}}, {AF::CountDistinct, {"w"}}, {AF::Sum, {"w"}}};
        const DataFrame g = Evaluate::group_aggregate(f, {"s", "k"}, aggs);
        CHECK(strings_of(g.column(0)) == (Opt<std::string>{std::string(""), std::string("a"), std::string("a"), std::string("a"), std::string("b"), std::string("b")}));
        CHECK(rows_of<int64_t>(g.column(1)) == (Opt<int64_t>{3, 1, 2, N, 1, N}));
        CHECK(rows_of<int64_t>(g.column_by_name("sum(w)")) == (Opt<int64_t>{32, 4, 2, 65, 16, 8}));
        CHECK(rows_of<uint32_t>(g.column_by_name("count_distinct(w)")) == (Opt<uint32_t>{1, 1, 1, 2, 1, 1}));
        CHECK(rows_of<int64_t>(g.column_by_name("last(w)")) == (Opt<int64_t>{32, 4, 2, 64, 16, 8}));
    }
}

TEST(sum_distinct_stays_unplanned) {
    CHECK_THROWS(Evaluate::group_aggregate(frame(), {"k"}, {{AF::SumDistinct, {"v"}}}));
}

int main() { return run_all(); }
