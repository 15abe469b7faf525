// ScalarFunctions::coalesce / greatest / least / nanvl / when(...).otherwise(...) / is_null / is_not_null / is_nan and the
// matching Column methods in the C++ mirror (rdf_frame.hpp -> rdf_coalesce / rdf_extremum / rdf_nanvl / rdf_case_when /
// rdf_null_test), run on the device over Array::from_vec columns.  The answers are Spark's documented examples and the tie,
// NaN and signed-zero rules of rdf_mi355x.h, written as literals.  Text columns go through rdf_utf8_coalesce / rdf_utf8_case_when,
// staged as concat stages its parts, and through rdf_null_test over their rows' bitmap.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using SF = ScalarFunctions;

template <class T> static std::vector<T> host(const ArrayRef& a) { return a->values_to_host<T>(); }
template <class T> static std::vector<ArrayRef> col(const std::vector<T>& v, const std::vector<bool>* valid = nullptr) { return {Array::from_vec<T>(v, valid)}; }
static std::vector<int32_t> I(std::initializer_list<int32_t> v) { return std::vector<int32_t>(v); }
static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

TEST(spark_examples) {
    const std::vector<bool> none = {false};
    // greatest(10, 9, 2, 4, 3) = 10, least(10, 9, 2, 4, 3) = 2
    const std::vector<SF::Value> five = {col<int32_t>({10}), Scalar(9), col<int32_t>({2}), Scalar(4), col<int32_t>({3})};
    CHECK_EQ(host<int32_t>(SF::greatest(five)[0]), I({10}));
    CHECK_EQ(host<int32_t>(SF::least(five)[0]), I({2}));
    // coalesce(NULL, 1, NULL) = 1
    const auto c = SF::coalesce({col<int32_t>({7}, &none), Scalar(1), Scalar()});
    CHECK_EQ(host<int32_t>(c[0]), I({1}));
    CHECK_EQ(c[0]->null_count, (int64_t)0);
    // nanvl(NaN, 123) = 123.0
    CHECK_EQ(host<double>(SF::nanvl(col<double>({kNaN, 2.5}), Scalar(123.0))[0]), std::vector<double>({123.0, 2.5}));
}

TEST(coalesce_and_fill_null_keep_bits_and_count_nulls) {
    const std::vector<bool> va = {true, false, false, true}, vb = {true, true, false, false};
    const auto a = col<double>({-0.0, 1.0, 2.0, 3.0}, &va), b = col<double>({9.0, 8.0, 7.0, 6.0}, &vb);
    const auto c = SF::coalesce({a, b});
    CHECK_EQ(host<double>(c[0]), std::vector<double>({-0.0, 8.0, 0.0, 3.0}));                  // (a NULL row holds 0)
    CHECK_EQ(bits(host<double>(c[0])[0]), bits(-0.0));
    CHECK(c[0]->valid_to_host() == std::vector<bool>({true, true, false, true}));
    CHECK_EQ(c[0]->null_count, (int64_t)1);
    const Column x = Column::from_arrays(a, Field{"x", DataType::Float64, true}), y = Column::from_arrays(b, Field{"y", DataType::Float64, true});
    const Column filled = x.fill_null(Scalar(0.5));
    CHECK_EQ(filled.data().chunk(0)->values_to_host<double>(), std::vector<double>({-0.0, 0.5, 0.5, 3.0}));
    CHECK_EQ(filled.null_count(), (int64_t)0);
    CHECK_EQ(x.coalesce(y).null_count(), (int64_t)1);
    CHECK_EQ(x.fill_null(Scalar(2)).data().chunk(0)->values_to_host<double>()[1], 2.0);        // an integer literal for a Float64 column
}

TEST(extremum_ties_nan_and_signed_zero) {
    const auto a = col<double>({kNaN, kNaN, -0.0, 0.0, 1.0}), b = col<double>({1.0, 1.0, 0.0, -0.0, kNaN});
    const auto g = host<double>(SF::greatest({a, b})[0]), l = host<double>(SF::least({a, b})[0]);
    CHECK(std::isnan(g[0]) && l[0] == 1.0);                                                    // greatest(NaN, 1) = NaN, least(NaN, 1) = 1
    CHECK_EQ(bits(g[2]), bits(-0.0));                                                          // a tie: the leftmost part's bits
    CHECK_EQ(bits(l[2]), bits(-0.0));
    CHECK_EQ(bits(g[3]), bits(0.0));
    CHECK(std::isnan(g[4]) && l[4] == 1.0);
    // UInt64 above 2^63 is the greater; a NULL part is skipped
    const std::vector<bool> v = {true, false};
    const auto u = SF::greatest({col<uint64_t>({1, 5}), col<uint64_t>({(1ull << 63) + 5, 9}, &v)});
    CHECK_EQ(host<uint64_t>(u[0]), std::vector<uint64_t>({(1ull << 63) + 5, 5}));
    const Column x = Column::from_arrays(col<int32_t>({1, 7}), Field{"x", DataType::Int32, true}), y = Column::from_arrays(col<int32_t>({4, -7}), Field{"y", DataType::Int32, true});
    CHECK_EQ(x.greatest(y).data().chunk(0)->values_to_host<int32_t>(), I({4, 7}));
    CHECK_EQ(x.least(y).data().chunk(0)->values_to_host<int32_t>(), I({1, -7}));
}

TEST(when_otherwise) {
    const std::vector<bool> cvalid = {false, true, true, true};
    const std::vector<ArrayRef> c0 = {Array::from_bools({true, false, false, true}, &cvalid)}, c1 = {Array::from_bools({true, true, false, true})};
    const auto x = col<int32_t>({10, 20, 30, 40});
    // row 0: the first condition is NULL, the second holds; row 3: both hold, the first wins
    CHECK_EQ(host<int32_t>(SF::when(c0, Scalar(1)).when(c1, x).otherwise(Scalar(-1))[0]), I({10, 20, -1, 1}));
    const auto open = SF::when(c0, x).end();                                                   // no otherwise: NULL
    CHECK(open[0]->valid_to_host() == std::vector<bool>({false, false, false, true}));
    CHECK_EQ(open[0]->null_count, (int64_t)3);
    CHECK_EQ(host<int32_t>(SF::when(c1, Scalar()).otherwise(x)[0]), I({0, 0, 30, 0}));         // a chosen NULL literal
}

TEST(null_tests) {
    const std::vector<bool> v = {true, false, true};
    const auto a = col<double>({kNaN, kNaN, 1.0}, &v);
    CHECK(SF::is_null(a)[0]->bools_to_host() == std::vector<bool>({false, true, false}));
    CHECK(SF::is_not_null(a)[0]->bools_to_host() == v);
    CHECK(SF::is_nan(a)[0]->bools_to_host() == std::vector<bool>({true, false, false}));       // isnan(NULL) is false
    CHECK_EQ(SF::is_nan(a)[0]->null_count, (int64_t)0);
    const Column x = Column::from_arrays(a, Field{"x", DataType::Float64, true});
    CHECK(x.is_null().data().chunk(0)->bools_to_host() == std::vector<bool>({false, true, false}));
    CHECK(x.is_nan().data_type() == DataType::Boolean);
    CHECK_EQ(x.nanvl(Column::from_arrays(col<double>({5.0, 6.0, 7.0}), Field{"y", DataType::Float64, true})).data().chunk(0)->values_to_host<double>(), std::vector<double>({5.0, 0.0, 1.0}));
}

// a Utf8 array of the mirror (strings carried on the host) with a validity bitmap
static ArrayRef text(std::vector<std::string> rows, const std::vector<bool>* valid = nullptr) {
    auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(rows)));
    if (valid) {
        const std::vector<uint8_t> bits = pack_bits(*valid);
        a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
        check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
        a->null_count = 0;
        for (bool v : *valid) a->null_count += v ? 0 : 1;
    }
    return a;
}
static std::vector<std::string> S(std::initializer_list<const char*> v) { return std::vector<std::string>(v.begin(), v.end()); }

TEST(text_null_to_unknown) {
    const std::vector<bool> va = {true, false, true, false}, vb = {false, false, true, true};
    const std::vector<ArrayRef> a = {text(S({"Leeds", "x", "", "y"}), &va), text(S({}))}, b = {text(S({"p", "q", "York", "Bath"}), &vb), text(S({}))};
    const auto filled = SF::coalesce({a, Scalar("unknown")});                                  // NULL -> 'unknown'; an empty row is not NULL
    CHECK_EQ(filled.size(), (size_t)2);
    CHECK_EQ(*filled[0]->strings, S({"Leeds", "unknown", "", "unknown"}));
    CHECK(filled[0]->validity == nullptr);
    CHECK_EQ(filled[1]->length, (int64_t)0);
    const auto ab = SF::coalesce({a, b});
    CHECK_EQ(*ab[0]->strings, S({"Leeds", "", "", "Bath"}));                                   // (a NULL row is an empty string)
    CHECK(ab[0]->valid_to_host() == std::vector<bool>({true, false, true, true}));
    CHECK_EQ(ab[0]->null_count, (int64_t)1);
    CHECK_EQ(*SF::coalesce({a, Scalar(), b, Scalar("z")})[0]->strings, S({"Leeds", "z", "", "Bath"}));
    const Column city = Column::from_arrays(a, Field{"city", DataType::Utf8, true}), other = Column::from_arrays(b, Field{"other", DataType::Utf8, true});
    const Column f = city.fill_null(Scalar("unknown"));
    CHECK_EQ(*f.data().chunk(0)->strings, S({"Leeds", "unknown", "", "unknown"}));
    CHECK_EQ(f.null_count(), (int64_t)0);
    CHECK(f.data_type() == DataType::Utf8 && f.name() == "city");
    CHECK_EQ(city.coalesce(other).null_count(), (int64_t)1);
    CHECK(city.is_null().data().chunk(0)->bools_to_host() == std::vector<bool>({false, true, false, true}));
    CHECK(city.is_not_null().data().chunk(0)->bools_to_host() == va);
    CHECK(SF::is_null(a)[0]->bools_to_host() == std::vector<bool>({false, true, false, true}));
    CHECK_EQ(city.is_null().null_count(), (int64_t)0);
    CHECK_THROWS(city.fill_null(Scalar(1)));
    CHECK_THROWS(city.is_nan());
    CHECK_THROWS(SF::greatest({a, b}));
}

TEST(text_case_when_bucket_labels) {
    const std::vector<bool> cvalid = {false, true, true, true};
    const std::vector<ArrayRef> c0 = {Array::from_bools({true, false, false, true}, &cvalid)}, c1 = {Array::from_bools({true, true, false, true})};
    const std::vector<bool> vx = {true, true, true, false};
    const std::vector<ArrayRef> x = {text(S({"a", "bb", "ccc", "dddd"}), &vx)};
    // row 0: the first condition is NULL, the second holds; row 3: both hold, the first wins
    const auto label = SF::when(c0, Scalar("low")).when(c1, x).otherwise(Scalar("other"));
    CHECK_EQ(*label[0]->strings, S({"a", "bb", "other", "low"}));
    CHECK_EQ(label[0]->null_count, (int64_t)0);
    const auto open = SF::when(c1, x).end();                                                   // no otherwise: NULL; row 3 takes a NULL value
    CHECK(open[0]->valid_to_host() == std::vector<bool>({true, true, false, false}));
    CHECK_EQ(open[0]->null_count, (int64_t)2);
    CHECK_EQ(*SF::when(c1, Scalar()).otherwise(x)[0]->strings, S({"", "", "ccc", ""}));        // a chosen NULL literal
    // the label is an ordinary text column: concat takes it
    CHECK_EQ(*SF::concat({label, "!"})[0]->strings, S({"a!", "bb!", "other!", "low!"}));
    CHECK_THROWS(SF::when(x, Scalar("low")).otherwise(x));                                     // a condition that is not Boolean
    CHECK_THROWS(SF::when(c0, Scalar(1)).otherwise(x));                                        // a number for a text column
}

TEST(refusals) {
    CHECK_THROWS(SF::coalesce({Scalar(1), Scalar(2)}));                                        // no column part
    CHECK_THROWS(SF::coalesce({col<int32_t>({1}), col<double>({1.0})}));                       // two dtypes
    CHECK_THROWS(SF::greatest({col<int32_t>({1})}));                                           // one part
    CHECK_THROWS(SF::nanvl(col<int32_t>({1}), Scalar(1)));                                     // not a float type
    CHECK_THROWS(SF::is_nan(col<int32_t>({1})));
    CHECK_THROWS(SF::coalesce({col<int32_t>({1}), Scalar("text")}));                           // a String literal for a numeric column
    CHECK_THROWS(SF::when({Array::from_vec<int32_t>({1})}, Scalar(1)).otherwise(col<int32_t>({2})));   // a condition that is not Boolean
}

int main() { return run_all(); }
