// percentile / median / percentile_disc in the C++ mirror (rdf_frame.hpp -> rdf_groupby_percentile), run on the device: the
// AggregateFunctions and Column::median / quantile on small columns (empty and all-NULL included, numeric and Utf8), and
// Evaluate::group_percentile over an integer key with a NULL, over a Utf8 key, over two keys and with a Utf8 value, row for
// row against typed-in answers.
#include <cmath>
#include <optional>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
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
static std::string S(const char* s) { return std::string(s); }
static const rdf_percentile_call MEDIAN{RDF_PCT_CONT, 0, 0.5}, MAXIMUM{RDF_PCT_CONT, 0, 1.0}, DISC_HALF{RDF_PCT_DISC, 0, 0.5};

TEST(whole_column_percentiles_of_numeric_columns) {
    const std::vector<bool> valid{true, true, true, true, false, true, true};
    const Column v = num<int64_t>("v", {5, 7, 9, 5, 8, 9, 6}, &valid);                 // 5 5 6 7 9 9
    CHECK_EQ(*AGG::median(v), 6.5);
    CHECK_EQ(*v.median(), 6.5);
    CHECK_EQ(*AGG::percentile(v, 0.25), 5.25);                                          // pos 1.25: 0.75 * 5 + 0.25 * 6
    CHECK_EQ(*v.quantile(0.0), 5.0);
    CHECK_EQ(*v.quantile(1.0), 9.0);
    const auto ps = AGG::percentiles(v, {0.0, 0.5, 1.0, 0.9});
    CHECK(ps.size() == 4 && *ps[0] == 5.0 && *ps[1] == 6.5 && *ps[2] == 9.0 && *ps[3] == 9.0);
    CHECK(rows_of<int64_t>(*AGG::percentile_disc(v, 0.5)) == (Opt<int64_t>{6}));      // k = ceil(3.0) - 1 = 2
    CHECK(rows_of<int64_t>(*AGG::percentile_disc(v, 0.51)) == (Opt<int64_t>{7}));
    CHECK(rows_of<int64_t>(*AGG::percentile_disc(v, 0.0)) == (Opt<int64_t>{5}));
    const Column f = num<double>("f", {1.0, std::nan(""), -0.0, 0.0, INFINITY});
    CHECK(std::isnan(*AGG::percentile(f, 1.0)));                                         // NaN after +inf
    CHECK_EQ(*AGG::percentile(f, 0.75), INFINITY);
    CHECK(*AGG::percentile(f, 0.125) == 0.0 && !std::signbit(*AGG::percentile(f, 0.125)));   // between -0.0 and +0.0: peers, +0.0
    const Column f32 = num<float>("g", {1.5f, 2.5f});
    CHECK_EQ(*AGG::median(f32), 2.0);
    const Column u8 = num<uint8_t>("u", {255, 0, 7});
    CHECK_EQ(*AGG::median(u8), 7.0);
    CHECK_THROWS(AGG::percentile(v, 1.5));
    CHECK_THROWS(AGG::percentile(v, std::nan("")));
    CHECK_THROWS(AGG::percentile_disc(v, -0.1));
    CHECK_THROWS(AGG::percentiles(v, std::vector<double>(9, 0.5)));
}

TEST(whole_column_percentiles_of_empty_all_null_and_utf8_columns) {
    const Column e = num<int64_t>("e", {});
    CHECK(!AGG::median(e) && !e.quantile(0.3) && !AGG::percentile_disc(e, 0.5));
    const std::vector<bool> none{false, false, false};
    const Column n = num<int16_t>("n", {4, 5, 6}, &none);
    CHECK(!AGG::median(n) && !n.median() && !AGG::percentile_disc(n, 0.5));
    CHECK(!AGG::percentiles(n, {0.1, 0.9})[1]);
    const std::vector<bool> valid{true, true, false, true, true};
    const Column s = text("s", {"b", "", "zz", "b", "a"}, &valid);                      // "" a b b
    CHECK(strings_of(*AGG::percentile_disc(s, 0.0)) == (Opt<std::string>{S("")}));
    CHECK(strings_of(*AGG::percentile_disc(s, 0.5)) == (Opt<std::string>{S("a")}));
    CHECK(strings_of(*AGG::percentile_disc(s, 1.0)) == (Opt<std::string>{S("b")}));
    CHECK_THROWS(AGG::median(s));
    CHECK(!AGG::percentile_disc(text("z", {}), 0.5));
}

//  row   0    1    2     3    4     5     6
//  k     2    1    NULL  2    1     NULL  2
//  v     5    7    9     5    NULL  9     6
//  s     b    a    ""    b    c     x     a
static DataFrame frame() {
    const std::vector<bool> kvalid{true, true, false, true, true, false, true}, vvalid{true, true, true, true, false, true, true};
    return DataFrame::from_columns({num<int64_t>("k", {2, 1, 0, 2, 1, 0, 2}, &kvalid), num<int64_t>("v", {5, 7, 9, 5, 8, 9, 6}, &vvalid),
                                    text("s", {"b", "a", "", "b", "c", "x", "a"})});
}

TEST(group_percentile_over_an_integer_key_with_a_null) {
    const DataFrame g = Evaluate::group_percentile(frame(), {"k"}, "v", {MEDIAN, MAXIMUM, DISC_HALF});
    CHECK_EQ(g.num_columns(), (size_t)4);
    const char* names[] = {"k", "median(v)", "percentile(v, 1)", "percentile_disc(v, 0.5)"};
    const DataType types[] = {DataType::Int64, DataType::Float64, DataType::Float64, DataType::Int64};
    for (size_t c = 0; c < 4; ++c) { CHECK_EQ(g.column(c).name(), std::string(names[c])); CHECK(g.column(c).data_type() == types[c]); }
    CHECK(rows_of<int64_t>(g.column(0)) == (Opt<int64_t>{1, 2, N}));                    // ascending, the NULL group last
    CHECK(rows_of<double>(g.column(1)) == (Opt<double>{7.0, 5.0, 9.0}));
    CHECK(rows_of<double>(g.column(2)) == (Opt<double>{7.0, 6.0, 9.0}));
    CHECK(rows_of<int64_t>(g.column(3)) == (Opt<int64_t>{7, 5, 9}));
}

TEST(group_percentile_over_a_utf8_key_and_over_two_keys) {
    const DataFrame g = Evaluate::group_percentile(frame(), {"s"}, "v", {MEDIAN, MAXIMUM, DISC_HALF});
    CHECK(g.column(0).data_type() == DataType::Utf8);
    CHECK(strings_of(g.column(0)) == (Opt<std::string>{S(""), S("a"), S("b"), S("c"), S("x")}));
    CHECK(rows_of<double>(g.column(1)) == (Opt<double>{9.0, 6.5, 5.0, N, 9.0}));        // c holds nothing but a NULL v
    CHECK(rows_of<double>(g.column(2)) == (Opt<double>{9.0, 7.0, 5.0, N, 9.0}));
    CHECK(rows_of<int64_t>(g.column(3)) == (Opt<int64_t>{9, 6, 5, N, 9}));
    const DataFrame h = Evaluate::group_percentile(frame(), {"s", "k"}, "v", {MEDIAN});
    CHECK(strings_of(h.column(0)) == (Opt<std::string>{S(""), S("a"), S("a"), S("b"), S("c"), S("x")}));
    CHECK(rows_of<int64_t>(h.column(1)) == (Opt<int64_t>{N, 1, 2, 2, 1, N}));
    CHECK(rows_of<double>(h.column(2)) == (Opt<double>{9.0, 7.0, 6.0, 5.0, N, 9.0}));
}

TEST(group_percentile_of_a_utf8_value_and_without_keys) {
    const DataFrame g = Evaluate::group_percentile(frame(), {"k"}, "s", {DISC_HALF, rdf_percentile_call{RDF_PCT_DISC, 0, 1.0}});
    CHECK(g.column(1).data_type() == DataType::Utf8 && g.column(1).name() == "percentile_disc(s, 0.5)");
    CHECK(strings_of(g.column(1)) == (Opt<std::string>{S("a"), S("b"), S("")}));        // a c | a b b | "" x
    CHECK(strings_of(g.column(2)) == (Opt<std::string>{S("c"), S("b"), S("x")}));
    CHECK_THROWS(Evaluate::group_percentile(frame(), {"k"}, "s", {MEDIAN}));            // no interpolation of text
    const DataFrame w = Evaluate::group_percentile(frame(), {}, "v", {MEDIAN, DISC_HALF});
    CHECK_EQ(w.num_columns(), (size_t)2);
    CHECK(rows_of<double>(w.column(0)) == (Opt<double>{6.5}));
    CHECK(rows_of<int64_t>(w.column(1)) == (Opt<int64_t>{6}));
    CHECK_THROWS(Evaluate::group_percentile(frame(), {"k"}, "v", {}));
    CHECK_THROWS(Evaluate::group_percentile(frame(), {"k"}, "v", {rdf_percentile_call{RDF_PCT_CONT, 0, 2.0}}));
}

int main() { return run_all(); }
