// Text predicates in the C++ mirror (rdf_frame.hpp -> rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure): DataFrame::filter
// over Utf8 columns with String scalars, ScalarFunctions::length / locate / contains, on the device.
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using BF = BooleanFilter;
using SF = ScalarFunctions;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

static std::vector<std::string> strings_of(const DataFrame& df, const std::string& name) {
    std::vector<std::string> out;
    for (auto& a : df.column_by_name(name).data().chunks())
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
static std::vector<std::string> S(std::initializer_list<const char*> v) { return std::vector<std::string>(v.begin(), v.end()); }
static std::vector<int32_t> I(std::initializer_list<int32_t> v) { return std::vector<int32_t>(v); }
static std::vector<bool> B(std::initializer_list<bool> v) { return std::vector<bool>(v); }

TEST(a_string_literal_is_a_string_scalar) {
    CHECK(Scalar("Leeds").kind == Scalar::String);            // (it used to pick the bool constructor)
    CHECK(Scalar(std::string("Leeds")).kind == Scalar::String && Scalar("Leeds").s == "Leeds");
    CHECK(Scalar(true).kind == Scalar::Boolean && Scalar(1.5).kind == Scalar::Float64);
}

TEST(filter_city_equals) {
    const DataFrame df = DataFrame::from_csv(g_csv);
    CHECK_EQ(df.filter(BF::eq(BF::column("city"), BF::scalar("Leeds"))).num_rows(), (int64_t)0);   // the column holds "Leeds, West Yorkshire, UK"
    const DataFrame one = df.filter(BF::eq(BF::column("city"), BF::scalar("Leeds, West Yorkshire, UK")));
    CHECK_EQ(strings_of(one, "city"), S({"Leeds, West Yorkshire, UK"}));
    CHECK_EQ(one.num_columns(), df.num_columns());
    CHECK_NEAR(one.column_by_name("lat").data().chunk(0)->value<double>(0), 53.801277, 1e-12);
    CHECK_EQ(df.filter(BF::ne(BF::column("city"), BF::scalar("London, UK"))).num_rows(), df.num_rows() - 1);
    CHECK_EQ(strings_of(df.filter(BF::starts_with(BF::column("city"), BF::scalar("Leeds"))), "city"), S({"Leeds, West Yorkshire, UK"}));
    CHECK_EQ(strings_of(df.filter(BF::ends_with(BF::column("city"), BF::scalar("the UK"))), "city"),
             S({"Elgin, Scotland, the UK", "Stoke-on-Trent, Staffordshire, the UK", "Inverness, the UK"}));
    CHECK_EQ(strings_of(df.filter(BF::contains(BF::column("city"), BF::scalar("London"))), "city"), S({"London, UK", "Londonderry, Derry, UK"}));
}

TEST(like_joined_with_a_numeric_comparison) {
    const DataFrame df = DataFrame::from_csv(g_csv);
    // S% : Stoke-on-Trent 53.0, Solihull 52.4, Swindon 51.6, Sutton Coldfield 52.6, Swansea 51.6, Salisbury 51.1
    const auto like_s = BF::like(BF::column("city"), BF::scalar("S%"));
    CHECK_EQ(df.filter(like_s).num_rows(), (int64_t)6);
    const DataFrame north = df.filter(BF::and_(like_s, BF::gt(BF::column("lat"), BF::scalar(Scalar(52.0)))));
    CHECK_EQ(strings_of(north, "city"), S({"Stoke-on-Trent, Staffordshire, the UK", "Solihull, Birmingham, UK", "Sutton Coldfield, West Midlands, UK"}));
    const DataFrame either = df.filter(BF::or_(BF::like(BF::column("city"), BF::scalar("_y_,%")), BF::not_(BF::lt(BF::column("lat"), BF::scalar(Scalar(57.6))))));
    CHECK_EQ(strings_of(either, "city"), S({"Elgin, Scotland, the UK", "Ayr, South Ayrshire, UK"}));
    // an escaped '%' is a literal: no city holds one
    CHECK_EQ(df.filter(BF::like(BF::column("city"), BF::scalar("S#%"), '#')).num_rows(), (int64_t)0);
    CHECK_THROWS(df.filter(BF::like(BF::column("city"), BF::scalar("S#"), '#')));          // a lone escape
}

TEST(a_scalar_on_the_left_flips_the_comparison) {
    const DataFrame df = DataFrame::from_csv(g_csv);
    const int64_t below = df.filter(BF::lt(BF::column("city"), BF::scalar("C"))).num_rows();        // Aberdeen, Ayr, Bournemouth, Bedford, Basildon, Belfast
    CHECK_EQ(below, (size_t)6);
    CHECK_EQ(df.filter(BF::gt(BF::scalar("C"), BF::column("city"))).num_rows(), below);
    CHECK_EQ(df.filter(BF::le(BF::scalar("C"), BF::column("city"))).num_rows(), df.num_rows() - below);
    CHECK_EQ(df.filter(BF::eq(BF::scalar("London, UK"), BF::column("city"))).num_rows(), (int64_t)1);
}

TEST(two_text_columns) {
    const std::vector<bool> valid = {true, true, false, true, true};
    auto with_nulls = std::make_shared<Array>(*Array::from_strings({"a", "b", "", "é", "zz"}));
    with_nulls->validity = Array::from_bools(valid, nullptr)->values;
    with_nulls->null_count = 1;
    const DataFrame df = DataFrame::from_columns({
        Column::from_arrays({with_nulls}, Field{"x", DataType::Utf8, true}),
        Column::from_arrays({Array::from_strings({"a", "a", "c", "z", "zzz"})}, Field{"y", DataType::Utf8, false}),
        Column::from_arrays({Array::from_vec<int64_t>({1, 2, 3, 4, 5})}, Field{"n", DataType::Int64, false})});
    auto ids = [](const DataFrame& d) { std::vector<int64_t> out; for (auto& a : d.column_by_name("n").data().chunks()) for (auto v : a->values_to_host<int64_t>()) out.push_back(v); return out; };
    CHECK_EQ(ids(df.filter(BF::eq(BF::column("x"), BF::column("y")))), (std::vector<int64_t>{1}));
    CHECK_EQ(ids(df.filter(BF::gt(BF::column("x"), BF::column("y")))), (std::vector<int64_t>{2, 4}));   // "é" > "z" in byte order; the NULL row is dropped
    CHECK_EQ(ids(df.filter(BF::lt(BF::column("x"), BF::column("y")))), (std::vector<int64_t>{5}));      // a proper prefix sorts first
    CHECK_EQ(ids(df.filter(BF::and_(BF::ge(BF::column("x"), BF::column("y")), BF::gt(BF::column("n"), BF::scalar(Scalar((int64_t)1)))))), (std::vector<int64_t>{2, 4}));
}

TEST(scalar_functions_over_text) {
    const std::vector<ArrayRef> s = {Array::from_strings({"abc", "", "aé😀", "xabcabc"}), Array::from_strings({"😀b"})};
    auto ints = [](const std::vector<ArrayRef>& r) { std::vector<int32_t> out; for (auto& a : r) for (auto v : a->values_to_host<int32_t>()) out.push_back(v); return out; };
    auto bools = [](const std::vector<ArrayRef>& r) { std::vector<bool> out; for (auto& a : r) for (bool v : a->bools_to_host()) out.push_back(v); return out; };
    CHECK_EQ(ints(SF::length(s)), I({3, 0, 3, 7, 2}));
    CHECK_EQ(ints(SF::octet_length(s)), I({3, 0, 7, 7, 5}));
    CHECK_EQ(ints(SF::instr(s, "bc")), I({2, 0, 0, 3, 0}));
    CHECK_EQ(ints(SF::locate("bc", s, 4)), I({0, 0, 0, 6, 0}));
    CHECK_EQ(ints(SF::locate("", s, 4)), I({4, 0, 4, 4, 0}));        // the empty needle is found wherever the row reaches
    CHECK_EQ(ints(SF::locate("😀", s)), I({0, 0, 3, 0, 1}));
    CHECK(bools(SF::contains(s, "abc")) == B({true, false, false, true, false}));
    CHECK(bools(SF::starts_with(s, "a")) == B({true, false, true, false, false}));
    CHECK(bools(SF::ends_with(s, "b")) == B({false, false, false, false, true}));
    CHECK(bools(SF::like(s, "_b%")) == B({true, false, false, false, true}));
    CHECK_EQ(SF::length(s)[0]->dtype, DataType::Int32);
    CHECK_EQ(SF::contains(s, "a")[1]->dtype, DataType::Boolean);
    CHECK_THROWS(SF::length({Array::from_vec<int64_t>({1})}));
}

TEST(text_against_a_number_still_throws) {
    const DataFrame df = DataFrame::from_csv(g_csv);
    CHECK_THROWS(df.filter(BF::eq(BF::column("city"), BF::scalar(Scalar(1.0)))));
    CHECK_THROWS(df.filter(BF::eq(BF::column("lat"), BF::scalar("Leeds"))));
    CHECK_THROWS(df.filter(BF::like(BF::column("lat"), BF::scalar("5%"))));
    CHECK_THROWS(df.filter(BF::starts_with(BF::column("city"), BF::column("city"))));
    CHECK_THROWS(df.filter(BF::eq(BF::column("town"), BF::scalar("Leeds"))));
}

int main() { return run_all(); }
