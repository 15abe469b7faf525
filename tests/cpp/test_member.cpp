// Semi / anti join, is_in, distinct rows and INTERSECT / EXCEPT in the C++ mirror (rdf_frame.hpp -> rdf_member_mask,
// rdf_first_occurrence), run on the device against typed-in answers on a dozen rows.
#include <optional>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;

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
static std::vector<std::optional<bool>> bools_of(const Column& c) {
    std::vector<std::optional<bool>> out;
    for (auto& a : c.data().chunks()) {
        const auto v = a->bools_to_host(), ok = a->valid_to_host();
        for (size_t r = 0; r < v.size(); ++r) out.push_back(ok[r] ? std::optional<bool>(v[r]) : std::nullopt);
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
using JT = DataFrame::JoinType;

//  row   0    1    2     3    4     5     6    7
//  k     2    1    NULL  2    3     NULL  5    1
//  s     b    a    ""    b    c     x     a    NULL
//  id    0    1    2     3    4     5     6    7
static DataFrame left() {
    const std::vector<bool> kvalid{true, true, false, true, true, false, true, true}, svalid{true, true, true, true, true, true, true, false};
    return DataFrame::from_columns({num<int64_t>("k", {2, 1, 0, 2, 3, 0, 5, 1}, &kvalid), text("s", {"b", "a", "", "b", "c", "x", "a", ""}, &svalid),
                                    num<int32_t>("id", {0, 1, 2, 3, 4, 5, 6, 7})});
}
//  rk    2    2    NULL  9    5
//  rs    b    zz   ""    a    NULL
static DataFrame right() {
    const std::vector<bool> kvalid{true, true, false, true, true}, svalid{true, true, true, true, false};
    return DataFrame::from_columns({num<int64_t>("rk", {2, 2, 0, 9, 5}, &kvalid), text("rs", {"b", "zz", "", "a", ""}, &svalid)});
}

TEST(left_semi_and_left_anti_keep_the_left_columns_only) {
    const DataFrame l = left(), r = right();
    const DataFrame semi = l.join(r, {JT::LeftSemi, {{"k", "rk"}}});
    CHECK_EQ(semi.num_columns(), (size_t)3);
    CHECK(rows_of<int32_t>(semi.column_by_name("id")) == (Opt<int32_t>{0, 3, 6}));        // duplicates on the right do not multiply rows
    CHECK(rows_of<int64_t>(semi.column_by_name("k")) == (Opt<int64_t>{2, 2, 5}));
    CHECK(strings_of(semi.column_by_name("s")) == (Opt<Str>{Str("b"), Str("b"), Str("a")}));
    const DataFrame anti = l.join(r, {JT::LeftAnti, {{"k", "rk"}}});
    CHECK(rows_of<int32_t>(anti.column_by_name("id")) == (Opt<int32_t>{1, 2, 4, 5, 7}));  // NULL keys are kept
    // a text criterion: "" is a value and matches "", NULL matches nothing
    CHECK(rows_of<int32_t>(l.join(r, {JT::LeftSemi, {{"s", "rs"}}}).column_by_name("id")) == (Opt<int32_t>{0, 1, 2, 3, 6}));
    CHECK(rows_of<int32_t>(l.join(r, {JT::LeftAnti, {{"s", "rs"}}}).column_by_name("id")) == (Opt<int32_t>{4, 5, 7}));
    // two criteria, numeric and text
    CHECK(rows_of<int32_t>(l.join(r, {JT::LeftSemi, {{"k", "rk"}, {"s", "rs"}}}).column_by_name("id")) == (Opt<int32_t>{0, 3}));
    CHECK(rows_of<int32_t>(l.join(r, {JT::LeftAnti, {{"k", "rk"}, {"s", "rs"}}}).column_by_name("id")) == (Opt<int32_t>{1, 2, 4, 5, 6, 7}));
}

TEST(is_in_is_three_valued) {
    const DataFrame l = left(), r = right();
    // the set holds a NULL: no match gives NULL, a NULL row gives NULL
    CHECK(bools_of(l.column_by_name("k").is_in(r.column_by_name("rk"))) == (Opt<bool>{true, N, N, true, N, N, true, N}));
    const Column set = num<int64_t>("set", {1, 3});
    CHECK(bools_of(l.column_by_name("k").is_in(set)) == (Opt<bool>{false, true, N, false, true, N, false, true}));
    CHECK(bools_of(l.column_by_name("k").is_in(num<int64_t>("none", {}))) == (Opt<bool>(8, false)));   // x IN () is FALSE, NULL rows included
    CHECK(bools_of(l.column_by_name("s").is_in(text("set", {"a", ""}))) == (Opt<bool>{false, true, true, false, false, false, true, N}));
    // filter(is_in): NULL drops the row like FALSE; NOT IN through not_
    const FilterRef in = BooleanFilter::is_in(BooleanFilter::column("k"), set);
    CHECK(rows_of<int32_t>(l.filter(in).column_by_name("id")) == (Opt<int32_t>{1, 4, 7}));
    CHECK(rows_of<int32_t>(l.filter(BooleanFilter::not_(in)).column_by_name("id")) == (Opt<int32_t>{0, 3, 6}));
    CHECK(rows_of<int32_t>(l.filter(BooleanFilter::and_(in, BooleanFilter::gt(BooleanFilter::column("id"), BooleanFilter::scalar(Scalar((int32_t)1))))).column_by_name("id")) == (Opt<int32_t>{4, 7}));
}

TEST(drop_duplicates_and_distinct) {
    const DataFrame l = left();
    using K = DataFrame::Keep;
    CHECK(rows_of<int32_t>(l.drop_duplicates({"k"}).column_by_name("id")) == (Opt<int32_t>{0, 1, 2, 4, 6}));          // NULL is one key
    CHECK(rows_of<int32_t>(l.drop_duplicates({"k"}, K::Last).column_by_name("id")) == (Opt<int32_t>{3, 4, 5, 6, 7}));
    CHECK(rows_of<int32_t>(l.drop_duplicates({"k"}, K::None).column_by_name("id")) == (Opt<int32_t>{4, 6}));
    CHECK(rows_of<int32_t>(l.drop_duplicates({"k", "s"}).column_by_name("id")) == (Opt<int32_t>{0, 1, 2, 4, 5, 6, 7}));
    CHECK(rows_of<int32_t>(l.drop_duplicates({"s"}, K::Last).column_by_name("id")) == (Opt<int32_t>{2, 3, 4, 5, 6, 7}));
    const DataFrame ks = DataFrame::from_columns({l.column_by_name("k"), l.column_by_name("s")});
    const DataFrame d = ks.distinct();
    CHECK(rows_of<int64_t>(d.column_by_name("k")) == (Opt<int64_t>{2, 1, N, 3, N, 5, 1}));
    // (the frame filter carries a text column's rows without their bitmap: a kept NULL text row reads as "")
    CHECK(strings_of(d.column_by_name("s")) == (Opt<Str>{Str("b"), Str("a"), Str(""), Str("c"), Str("x"), Str("a"), Str("")}));
    CHECK_EQ(l.distinct().num_rows(), (int64_t)8);
}

TEST(intersect_and_except_are_distinct_and_null_safe) {
    //  a: (2,b) (1,a) (NULL,"") (2,b) (3,c) (NULL,"") (5,NULL) (1,a)
    //  b: (2,b) (2,b) (NULL,"") (9,a) (5,NULL) (1,zz)
    const std::vector<bool> akv{true, true, false, true, true, false, true, true}, asv{true, true, true, true, true, true, false, true};
    const std::vector<bool> bkv{true, true, false, true, true, true}, bsv{true, true, true, true, false, true};
    const DataFrame a = DataFrame::from_columns({num<int64_t>("k", {2, 1, 0, 2, 3, 0, 5, 1}, &akv), text("s", {"b", "a", "", "b", "c", "", "", "a"}, &asv)});
    const DataFrame b = DataFrame::from_columns({num<int64_t>("x", {2, 2, 0, 9, 5, 1}, &bkv), text("y", {"b", "b", "", "a", "", "zz"}, &bsv)});
    const DataFrame i = a.intersect(b);
    CHECK(rows_of<int64_t>(i.column_by_name("k")) == (Opt<int64_t>{2, N, 5}));              // NULL equals NULL here, unlike SEMI
    CHECK(strings_of(i.column_by_name("s")) == (Opt<Str>{Str("b"), Str(""), Str("")}));   // (5, NULL): the filter keeps the row, its text reads as ""
    const DataFrame e = a.except(b);
    CHECK(rows_of<int64_t>(e.column_by_name("k")) == (Opt<int64_t>{1, 3}));
    CHECK(strings_of(e.column_by_name("s")) == (Opt<Str>{Str("a"), Str("c")}));
    CHECK_EQ(b.except(a).num_rows(), (int64_t)2);                                            // (9,a) (1,zz)
    CHECK_EQ(a.intersect(a).num_rows(), (int64_t)5);
    CHECK_EQ(a.except(a).num_rows(), (int64_t)0);
}

TEST(more_than_four_key_columns_is_an_error_that_says_so) {
    std::vector<Column> cols;
    for (int k = 0; k < 5; ++k) cols.push_back(num<int32_t>("c" + std::to_string(k), {1, 2, 1}));
    const DataFrame f = DataFrame::from_columns(cols);
    bool said = false;
    try { f.distinct(); } catch (const DataFrameError& e) { said = std::string(e.what()).find("more than 4 key columns") != std::string::npos; }
    CHECK(said);
    CHECK_THROWS(f.intersect(f));
    CHECK_THROWS(f.except(f));
    CHECK_THROWS(f.drop_duplicates({"c0", "c1", "c2", "c3", "c4"}));
    CHECK_EQ(f.drop_duplicates({"c0", "c1", "c2", "c3"}).num_rows(), (int64_t)2);
}

int main() { return run_all(); }
