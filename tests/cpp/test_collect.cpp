// collect_list / collect_set / explode in the C++ mirror (rdf_frame.hpp -> rdf_groupby_collect, rdf_list_explode), run on the
// device: Evaluate::group_collect over an integer key with a NULL and over a Utf8 key, lined up row for row with
// Evaluate::group_aggregate(Count) on the same frame; explode / explode_outer / posexplode of a frame with a numeric and a
// Utf8 passenger column; the no-grouping ArrayFunctions::collect_list / collect_set.  Against typed-in answers.
#include <cmath>
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
using Str = std::string;
static const std::nullopt_t N = std::nullopt;

//  row   0    1    2     3    4     5     6
//  k     2    1    NULL  2    1     NULL  2
//  v     5    7    9     5    NULL  9     6
//  s     b    a    ""    b    c     x     a
static DataFrame frame() {
    const std::vector<bool> kvalid{true, true, false, true, true, false, true}, vvalid{true, true, true, true, false, true, true};
    return DataFrame::from_columns({num<int64_t>("k", {2, 1, 0, 2, 1, 0, 2}, &kvalid), num<int64_t>("v", {5, 7, 9, 5, 8, 9, 6}, &vvalid),
                                    text("s", {"b", "a", "", "b", "c", "x", "a"})});
}

TEST(group_collect_over_an_integer_key_lines_up_with_count) {
    const DataFrame f = frame();
    const DataFrame counts = Evaluate::group_aggregate(f, {"k"}, {{AF::Count, {"v"}}});
    const GroupedLists l = Evaluate::group_collect(f, {"k"}, "v", RDF_COLLECT_LIST);
    CHECK_EQ(l.groups(), (int64_t)3);
    CHECK(rows_of<int64_t>(l.keys.column(0)) == rows_of<int64_t>(counts.column(0)));       // 1, 2, NULL
    CHECK(rows_of<int64_t>(l.keys.column(0)) == (Opt<int64_t>{1, 2, N}));
    CHECK((l.lists().rows_to_host<int64_t>() == std::vector<std::vector<int64_t>>{{7}, {5, 5, 6}, {9, 9}}));   // row order, the NULL v dropped
    const auto cnt = rows_of<uint32_t>(counts.column_by_name("count(v)"));
    for (int64_t g = 0; g < l.groups(); ++g) CHECK_EQ((int64_t)l.lists().value_length(g), (int64_t)*cnt[(size_t)g]);
    const GroupedLists s = Evaluate::group_collect(f, {"k"}, "v", RDF_COLLECT_SET);
    CHECK((s.lists().rows_to_host<int64_t>() == std::vector<std::vector<int64_t>>{{7}, {5, 6}, {9}}));
    // a Utf8 value: offsets plus a text child
    const GroupedLists t = Evaluate::group_collect(f, {"k"}, "s", RDF_COLLECT_SET);
    CHECK((t.offsets->values_to_host<int32_t>() == std::vector<int32_t>{0, 2, 4, 6}));
    CHECK(strings_of(t.child) == (Opt<Str>{Str("a"), Str("c"), Str("a"), Str("b"), Str(""), Str("x")}));
    CHECK(t.child.data_type() == DataType::Utf8 && t.child.name() == "s");
    CHECK_THROWS(t.lists());
    const GroupedLists tl = Evaluate::group_collect(f, {"k"}, "s", RDF_COLLECT_LIST);
    CHECK(strings_of(tl.child) == (Opt<Str>{Str("a"), Str("c"), Str("b"), Str("b"), Str("a"), Str(""), Str("x")}));
}

TEST(group_collect_over_a_utf8_key_and_two_keys) {
    const DataFrame f = frame();
    const DataFrame counts = Evaluate::group_aggregate(f, {"s"}, {{AF::Count, {"v"}}});
    const GroupedLists l = Evaluate::group_collect(f, {"s"}, "v", RDF_COLLECT_LIST);
    CHECK(strings_of(l.keys.column(0)) == strings_of(counts.column(0)));
    CHECK(strings_of(l.keys.column(0)) == (Opt<Str>{Str(""), Str("a"), Str("b"), Str("c"), Str("x")}));
    CHECK((l.lists().rows_to_host<int64_t>() == std::vector<std::vector<int64_t>>{{9}, {7, 6}, {5, 5}, {}, {9}}));   // "c" holds only a NULL v: an empty list
    const auto cnt = rows_of<uint32_t>(counts.column_by_name("count(v)"));
    for (int64_t g = 0; g < l.groups(); ++g) CHECK_EQ((int64_t)l.lists().value_length(g), (int64_t)*cnt[(size_t)g]);
    const GroupedLists two = Evaluate::group_collect(f, {"s", "k"}, "v", RDF_COLLECT_SET);
    CHECK(strings_of(two.keys.column(0)) == (Opt<Str>{Str(""), Str("a"), Str("a"), Str("b"), Str("c"), Str("x")}));
    CHECK(rows_of<int64_t>(two.keys.column(1)) == (Opt<int64_t>{N, 1, 2, 2, 1, N}));
    CHECK((two.lists().rows_to_host<int64_t>() == std::vector<std::vector<int64_t>>{{9}, {7}, {6}, {5}, {}, {9}}));
    const GroupedLists all = Evaluate::group_collect(f, {}, "v", RDF_COLLECT_SET);         // no grouping columns: one group
    CHECK_EQ(all.keys.num_columns(), (size_t)0);
    CHECK((all.lists().rows_to_host<int64_t>() == std::vector<std::vector<int64_t>>{{5, 6, 7, 9}}));
}

TEST(collect_list_and_collect_set_of_a_whole_column) {
    const std::vector<bool> valid{true, true, false, true, true, true};
    const Column c = num<double>("c", {2.5, -0.0, 7.0, 0.0, 2.5, -1.0}, &valid);
    CHECK((ArrayFunctions::collect_list(c).rows_to_host<double>() == std::vector<std::vector<double>>{{2.5, -0.0, 0.0, 2.5, -1.0}}));
    const ListArray s = ArrayFunctions::collect_set(c);
    CHECK_EQ(s.len(), (int64_t)1);
    const auto rows = s.rows_to_host<double>();
    CHECK((rows == std::vector<std::vector<double>>{{-1.0, 0.0, 2.5}}));
    CHECK(!std::signbit(rows[0][1]));                                                      // either zero comes out as +0.0
    const Column e = num<int32_t>("e", {});
    CHECK((ArrayFunctions::collect_list(e).rows_to_host<int32_t>() == std::vector<std::vector<int32_t>>{{}}));
    const std::vector<bool> none{false, false};
    CHECK((ArrayFunctions::collect_set(num<int16_t>("n", {4, 5}, &none)).rows_to_host<int16_t>() == std::vector<std::vector<int16_t>>{{}}));
    CHECK_THROWS(ArrayFunctions::collect_list(text("t", {"a"})));
}

//  row    0        1      2     3        4
//  id     10       11     12    13       14
//  name   a        b      c     NULL     e
//  list   [1, 2]   NULL   []    [3]      [4, 5, 6]
TEST(explode_explode_outer_and_posexplode) {
    const std::vector<bool> nvalid{true, true, true, false, true};
    const DataFrame f = DataFrame::from_columns({num<int32_t>("id", {10, 11, 12, 13, 14}), text("name", {"a", "b", "c", "", "e"}, &nvalid)});
    const ListArray list = ListArray::from_rows<int64_t>({std::vector<int64_t>{1, 2}, std::nullopt, std::vector<int64_t>{}, std::vector<int64_t>{3}, std::vector<int64_t>{4, 5, 6}});
    const DataFrame x = ScalarFunctions::explode(f, list, "x");
    CHECK_EQ(x.num_columns(), (size_t)3);
    CHECK(rows_of<int32_t>(x.column_by_name("id")) == (Opt<int32_t>{10, 10, 13, 14, 14, 14}));
    CHECK(strings_of(x.column_by_name("name")) == (Opt<Str>{Str("a"), Str("a"), N, Str("e"), Str("e"), Str("e")}));
    CHECK(rows_of<int64_t>(x.column_by_name("x")) == (Opt<int64_t>{1, 2, 3, 4, 5, 6}));
    const DataFrame o = ScalarFunctions::explode_outer(f, list, "x");
    CHECK(rows_of<int32_t>(o.column_by_name("id")) == (Opt<int32_t>{10, 10, 11, 12, 13, 14, 14, 14}));
    CHECK(strings_of(o.column_by_name("name")) == (Opt<Str>{Str("a"), Str("a"), Str("b"), Str("c"), N, Str("e"), Str("e"), Str("e")}));
    CHECK(rows_of<int64_t>(o.column_by_name("x")) == (Opt<int64_t>{1, 2, N, N, 3, 4, 5, 6}));
    const DataFrame p = ScalarFunctions::posexplode(f, list, "pos", "x");
    CHECK_EQ(p.num_columns(), (size_t)4);
    CHECK(p.column(2).name() == "pos" && p.column(2).data_type() == DataType::Int32 && p.column(3).name() == "x");
    CHECK(rows_of<int32_t>(p.column_by_name("pos")) == (Opt<int32_t>{0, 1, 0, 0, 1, 2}));
    const DataFrame po = ScalarFunctions::posexplode(f, list, "pos", "x", true);
    CHECK(rows_of<int32_t>(po.column_by_name("pos")) == (Opt<int32_t>{0, 1, N, N, 0, 0, 1, 2}));
    CHECK(rows_of<int64_t>(po.column_by_name("x")) == (Opt<int64_t>{1, 2, N, N, 3, 4, 5, 6}));
    // explode inverts collect_list: the lists of group_collect exploded over their keys give the rows back, NULL v dropped
    const GroupedLists l = Evaluate::group_collect(frame(), {"k"}, "v", RDF_COLLECT_LIST);
    const DataFrame back = ScalarFunctions::explode(l.keys, l.lists(), "v");
    CHECK(rows_of<int64_t>(back.column_by_name("k")) == (Opt<int64_t>{1, 2, 2, 2, N, N}));
    CHECK(rows_of<int64_t>(back.column_by_name("v")) == (Opt<int64_t>{7, 5, 5, 6, 9, 9}));
    CHECK_THROWS(ScalarFunctions::explode(frame(), list, "x"));                            // 7 rows against 5 lists
}

int main() { return run_all(); }
