// Variance / stddev / skewness / kurtosis / covar / corr per group in the C++ mirror (rdf_frame.hpp -> rdf_groupby_moments),
// run on the device: Evaluate::group_moments / group_comoments against values worked out here, and a GroupAggregate step that
// mixes Sum, CountDistinct and StdDev — three paths, one group order — over sparse keys, dense small keys (the dense, fused
// and multi fast paths decline the moment functions), a Utf8 key and a host-resident frame, row for row.
#include <cmath>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
namespace P = rdf::plan;
using AF = P::AggregateFunction;

template <class T> static Column num(const std::string& name, const std::vector<T>& v, const std::vector<bool>* valid = nullptr) {
    return Column::from_arrays({Array::from_vec<T>(v, valid)}, Field{name, TypeOf<T>::value, true});
}
// the same column in page-locked host memory: a host-resident frame
template <class T> static Column host_num(const std::string& name, const std::vector<T>& v, const std::vector<bool>* valid = nullptr) {
    auto a = Array::make_out(TypeOf<T>::value, (int64_t)v.size(), valid != nullptr, true);
    std::memcpy(a->values->data(), v.data(), v.size() * sizeof(T));
    a->length = (int64_t)v.size();
    if (valid) {
        const auto bits = pack_bits(*valid);
        std::memcpy(a->validity->data(), bits.data(), bits.size());
        for (bool b : *valid) a->null_count += !b;
    }
    return Column::from_arrays({ArrayRef(a)}, Field{name, TypeOf<T>::value, true});
}
static Column text(const std::string& name, std::vector<std::string> rows) {
    return Column::from_arrays({Array::from_strings(std::move(rows))}, Field{name, DataType::Utf8, true});
}
template <class T> static std::vector<std::optional<T>> rows_of(const Column& c) {
    std::vector<std::optional<T>> out;
    for (auto& a : c.data().chunks()) {
        const auto v = a->values_to_host<T>();
        const auto ok = a->valid_to_host();
        for (size_t r = 0; r < v.size(); ++r) out.push_back(ok[r] ? std::optional<T>(v[r]) : std::nullopt);
    }
    return out;
}
static std::vector<std::string> strings_of(const Column& c) {
    std::vector<std::string> out;
    for (auto& a : c.data().chunks())
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
template <class T> using Opt = std::vector<std::optional<T>>;
static const std::nullopt_t N = std::nullopt;

// a column of doubles against worked-out values: NULLs in the same places, values within a few ulps
static bool close_to(const Column& c, const Opt<double>& want) {
    const Opt<double> got = rows_of<double>(c);
    if (c.data_type() != DataType::Float64 || got.size() != want.size()) return false;
    for (size_t r = 0; r < got.size(); ++r) {
        if (got[r].has_value() != want[r].has_value()) return false;
        if (got[r] && !(std::fabs(*got[r] - *want[r]) <= 8e-16 * std::fabs(*want[r]))) return false;
    }
    return true;
}

//  row   0    1   2     3    4   5     6    7
//  k     1e6  5   NULL  1e6  5   NULL  1e6  5          sparse: the hash GROUP BY
//  d     2    0   1     2    0   1     2    0          dense and small: the dense kernel's shape
//  s     c    a   b     c    a   b     c    a
//  x     1    2   4     3    6   4     8    NULL
//  y     2    1   0     6    5   1     7    9
//  w     1    2   4     8    16  32    64   128
// per group, in the order of every key: (5 | 0 | a) rows 1 4 7, (NULL | 1 | b) rows 2 5, (1e6 | 2 | c) rows 0 3 6 — by k the
// NULL group comes last.
//   rows 1 4 7: x = 2, 6 (one NULL): mean 4, M2 8, M3 0, M4 32: var 8, skewness 0, kurtosis 2 * 32 / 64 - 3 = -2
//   rows 2 5:   x = 4, 4: constant: var 0, stddev 0, skewness and kurtosis absent
//   rows 0 3 6: x = 1, 3, 8: mean 4, d = -3 -1 4: M2 26, M3 36, M4 338: var 13, skewness sqrt(3) 36 / 26^1.5, kurtosis 3 * 338 / 676 - 3 = -1.5
template <class MakeI64, class MakeF64>
static DataFrame frame(MakeI64 i64, MakeF64 f64, bool with_text) {
    const std::vector<bool> kvalid{true, true, false, true, true, false, true, true}, xvalid{true, true, true, true, true, true, true, false};
    std::vector<Column> cols{i64("k", std::vector<int64_t>{1000000, 5, 0, 1000000, 5, 0, 1000000, 5}, &kvalid),
                             i64("d", std::vector<int64_t>{2, 0, 1, 2, 0, 1, 2, 0}, nullptr),
                             f64("x", std::vector<double>{1, 2, 4, 3, 6, 4, 8, 0}, &xvalid),
                             f64("y", std::vector<double>{2, 1, 0, 6, 5, 1, 7, 9}, nullptr),
                             i64("w", std::vector<int64_t>{1, 2, 4, 8, 16, 32, 64, 128}, nullptr)};
    if (with_text) cols.push_back(text("s", {"c", "a", "b", "c", "a", "b", "c", "a"}));
    return DataFrame::from_columns(std::move(cols));
}
static DataFrame device_frame() { return frame(num<int64_t>, num<double>, true); }
static DataFrame host_frame() { return frame(host_num<int64_t>, host_num<double>, false); }

static const double SKEW_C = std::sqrt(3.0) * 36.0 / (26.0 * std::sqrt(26.0));

TEST(group_moments_against_worked_out_values) {
    const std::vector<int32_t> all{RDF_STAT_MEAN, RDF_STAT_VAR_POP, RDF_STAT_VAR_SAMP, RDF_STAT_STDDEV_POP, RDF_STAT_STDDEV_SAMP, RDF_STAT_SKEWNESS, RDF_STAT_KURTOSIS};
    const DataFrame g = Evaluate::group_moments(device_frame(), {"k"}, "x", all);
    CHECK_EQ(g.num_columns(), (size_t)8);
    const char* names[] = {"k", "mean(x)", "var_pop(x)", "var_samp(x)", "stddev_pop(x)", "stddev_samp(x)", "skewness(x)", "kurtosis(x)"};
    for (size_t c = 0; c < 8; ++c) CHECK_EQ(g.column(c).name(), std::string(names[c]));
    CHECK(rows_of<int64_t>(g.column(0)) == (Opt<int64_t>{5, 1000000, N}));                 // ascending, the NULL group last
    CHECK(close_to(g.column(1), {4.0, 4.0, 4.0}));
    CHECK(close_to(g.column(2), {4.0, 26.0 / 3.0, 0.0}));
    CHECK(close_to(g.column(3), {8.0, 13.0, 0.0}));
    CHECK(close_to(g.column(4), {2.0, std::sqrt(26.0 / 3.0), 0.0}));
    CHECK(close_to(g.column(5), {std::sqrt(8.0), std::sqrt(13.0), 0.0}));
    CHECK(close_to(g.column(6), {0.0, SKEW_C, N}));
    CHECK(close_to(g.column(7), {-2.0, -1.5, N}));
    // no grouping columns: the whole column is one group — rdf_moments' answer: x = 1 2 4 3 6 4 8: mean 4, M2 34
    const DataFrame one = Evaluate::group_moments(device_frame(), {}, "x", {RDF_STAT_VAR_SAMP, RDF_STAT_MEAN});
    CHECK_EQ(one.num_columns(), (size_t)2);
    CHECK(close_to(one.column(0), {34.0 / 6.0}) && close_to(one.column(1), {4.0}));
    CHECK(close_to(one.column(0), {*AggregateFunctions::variance(device_frame().column_by_name("x").data())}));
    // two keys, one of them text; an Int64 value column is read `as f64`: w of rows (1 4 7), (2 5), (0 3 6)
    const DataFrame two = Evaluate::group_moments(device_frame(), {"s", "d"}, "w", {RDF_STAT_MEAN, RDF_STAT_VAR_SAMP});
    CHECK(strings_of(two.column(0)) == (std::vector<std::string>{"a", "b", "c"}));
    CHECK(rows_of<int64_t>(two.column(1)) == (Opt<int64_t>{0, 1, 2}));
    CHECK(close_to(two.column(2), {146.0 / 3.0, 18.0, 73.0 / 3.0}));
    CHECK(close_to(two.column(3), {(2.0 * 2 + 16.0 * 16 + 128.0 * 128 - 146.0 * 146 / 3) / 2, 392.0, (1.0 + 64 + 4096 - 73.0 * 73 / 3) / 2}));
    CHECK_THROWS(Evaluate::group_moments(device_frame(), {"k"}, "x", {}));
    CHECK_THROWS(Evaluate::group_moments(device_frame(), {"k"}, "x", {7}));
    CHECK_THROWS(Evaluate::group_moments(device_frame(), {"k"}, "s", {RDF_STAT_MEAN}));   // a Utf8 value column
}

TEST(group_comoments_against_worked_out_values) {
    // rows 1 4 (row 7's x is NULL): x = 2 6, y = 1 5: dx = -2 2, dy = -2 2: Cxy 8, M2x 8, M2y 8: corr 1
    // rows 2 5: x constant: Cxy 0, corr absent
    // rows 0 3 6: x = 1 3 8, y = 2 6 7: dx = -3 -1 4, dy = -3 1 2: Cxy 9 - 1 + 8 = 16, M2x 26, M2y 14
    const DataFrame g = Evaluate::group_comoments(device_frame(), {"d"}, "x", "y", {RDF_COSTAT_COVAR_POP, RDF_COSTAT_COVAR_SAMP, RDF_COSTAT_CORR});
    const char* names[] = {"d", "covar_pop(x, y)", "covar_samp(x, y)", "corr(x, y)"};
    for (size_t c = 0; c < 4; ++c) CHECK_EQ(g.column(c).name(), std::string(names[c]));
    CHECK(rows_of<int64_t>(g.column(0)) == (Opt<int64_t>{0, 1, 2}));
    CHECK(close_to(g.column(1), {4.0, 0.0, 16.0 / 3.0}));
    CHECK(close_to(g.column(2), {8.0, 0.0, 8.0}));
    CHECK(close_to(g.column(3), {1.0, N, 16.0 / std::sqrt(26.0 * 14.0)}));
    CHECK_THROWS(Evaluate::group_comoments(device_frame(), {"d"}, "x", "y", {RDF_COSTAT_CORR + 1}));
}

// sum(w), count_distinct(w) and stddev(x) of one step: the hash path, the sorted path and the moments path, row for row
static void check_step(const DataFrame& f, const std::string& key, bool null_last) {
    const DataFrame g = Evaluate::group_aggregate(f, {key}, {{AF::Sum, {"w"}}, {AF::CountDistinct, {"w"}}, {AF::StdDev, {"x"}}});
    CHECK_EQ(g.num_columns(), (size_t)4);
    CHECK_EQ(g.column(1).name(), std::string("sum(w)"));
    CHECK_EQ(g.column(2).name(), std::string("count_distinct(w)"));
    CHECK_EQ(g.column(3).name(), std::string("stddev(x)"));
    if (null_last) {   // by k: 5, 1e6, NULL
        CHECK(rows_of<int64_t>(g.column(1)) == (Opt<int64_t>{146, 73, 36}));
        CHECK(close_to(g.column(3), {std::sqrt(8.0), std::sqrt(13.0), 0.0}));
    } else {           // by d or s: rows (1 4 7), (2 5), (0 3 6)
        CHECK(rows_of<int64_t>(g.column(1)) == (Opt<int64_t>{146, 36, 73}));
        CHECK(close_to(g.column(3), {std::sqrt(8.0), 0.0, std::sqrt(13.0)}));
    }
    CHECK(rows_of<uint32_t>(g.column(2)) == (null_last ? Opt<uint32_t>{3, 3, 2} : Opt<uint32_t>{3, 2, 3}));
    // the moment functions first: they then supply the key column; one call carries all four statistics of x
    const DataFrame m = Evaluate::group_aggregate(f, {key}, {{AF::Variance, {"x", "w"}}, {AF::Kurtosis, {"x"}}, {AF::Sum, {"w"}}, {AF::Skewness, {"x"}}, {AF::StdDev, {"x"}}});
    const char* names[] = {"variance(x)", "variance(w)", "kurtosis(x)", "sum(w)", "skewness(x)", "stddev(x)"};
    CHECK_EQ(m.num_columns(), (size_t)7);
    for (size_t c = 0; c < 6; ++c) CHECK_EQ(m.column(c + 1).name(), std::string(names[c]));
    if (null_last) {
        CHECK(close_to(m.column(1), {8.0, 13.0, 0.0}));
        CHECK(close_to(m.column(3), {-2.0, -1.5, N}));
        CHECK(rows_of<int64_t>(m.column(4)) == (Opt<int64_t>{146, 73, 36}));
        CHECK(close_to(m.column(5), {0.0, SKEW_C, N}));
    } else {
        CHECK(close_to(m.column(1), {8.0, 0.0, 13.0}));
        CHECK(close_to(m.column(3), {-2.0, N, -1.5}));
        CHECK(rows_of<int64_t>(m.column(4)) == (Opt<int64_t>{146, 36, 73}));
        CHECK(close_to(m.column(5), {0.0, N, SKEW_C}));
    }
}

TEST(a_step_of_sum_count_distinct_and_stddev_over_sparse_keys) {
    check_step(device_frame(), "k", true);
    CHECK(rows_of<int64_t>(Evaluate::group_aggregate(device_frame(), {"k"}, {{AF::StdDev, {"x"}}}).column(0)) == (Opt<int64_t>{5, 1000000, N}));
}

TEST(a_step_over_dense_small_keys_where_the_fast_paths_decline) {
    check_step(device_frame(), "d", false);
    // the fused dense path sees the step first when it comes through the evaluator's lazy state: it declines, and does not throw
    const DataFrame g = Evaluate::group_aggregate(device_frame(), {"d"}, {{AF::Sum, {"w"}}, {AF::Avg, {"w"}}, {AF::Variance, {"x"}}});
    CHECK(rows_of<int64_t>(g.column(0)) == (Opt<int64_t>{0, 1, 2}));
    CHECK(rows_of<int64_t>(g.column_by_name("sum(w)")) == (Opt<int64_t>{146, 36, 73}));
    CHECK(close_to(g.column_by_name("avg(w)"), {146.0 / 3.0, 18.0, 73.0 / 3.0}));
    CHECK(close_to(g.column_by_name("variance(x)"), {8.0, 0.0, 13.0}));
}

TEST(a_step_over_a_utf8_key) {
    check_step(device_frame(), "s", false);
    CHECK(strings_of(Evaluate::group_aggregate(device_frame(), {"s"}, {{AF::Kurtosis, {"x"}}}).column(0)) == (std::vector<std::string>{"a", "b", "c"}));
}

TEST(a_step_over_a_host_resident_frame) {
    const DataFrame h = host_frame();
    CHECK(h.is_host());
    check_step(h, "k", true);
    check_step(h, "d", false);
    CHECK(close_to(Evaluate::group_moments(h, {"k"}, "x", {RDF_STAT_KURTOSIS}).column(1), {-2.0, -1.5, N}));
}

TEST(the_plan_keeps_refusing_the_moment_functions) {
    CHECK_THROWS(LazyFrame::read(device_frame()).aggregate({"k"}, {{AF::StdDev, {"x"}}}));
    CHECK_THROWS(Evaluate::group_aggregate(device_frame(), {"k"}, {{AF::StdDev, {"s"}}}));   // a Utf8 value column
}

int main() { return run_all(); }
