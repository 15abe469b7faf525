// test_textfloat.cpp — Float32 / Float64 to and from text in the C++ mirror (include/rdf_frame.hpp): ScalarFunctions::cast between
// Utf8 and the float types, Column::cast_text, Column::utf8_parse_float and Column::utf8_format_float, held to literals taken from
// the model (tests/textfloat_ref.py).  Needs a GPU.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;

static std::vector<std::string> strings_of(const std::vector<ArrayRef>& chunks) {
    std::vector<std::string> out;
    for (auto& a : chunks)
        for (int64_t r = 0; r < a->length; ++r) out.push_back(a->is_null(r) ? std::string("<null>") : (*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
// the bits of every value, 0xdead for a NULL row
template <class T, class B>
static std::vector<unsigned long long> bits_of(const std::vector<ArrayRef>& chunks) {
    std::vector<unsigned long long> out;
    for (auto& a : chunks) {
        const std::vector<T> v = a->values_to_host<T>();
        const std::vector<bool> ok = a->valid_to_host();
        for (size_t r = 0; r < v.size(); ++r) {
            B b;
            std::memcpy(&b, &v[r], sizeof b);
            out.push_back(ok[r] ? (unsigned long long)b : 0xdeadull);
        }
    }
    return out;
}
static double f64_of(unsigned long long b) { double x; std::memcpy(&x, &b, 8); return x; }
static float f32_of(unsigned b) { float x; std::memcpy(&x, &b, 4); return x; }

static const std::vector<std::string> kTexts = {" 3.14", "1e5", ".5", "5.", "-0", "nan", "-Infinity", "1e999", "0x10", "1d", "", "9007199254740993",
                                                "9007199254740993.0000000000000000000000000000001", "2.4703282292062328e-324"};

TEST(cast_text_to_float64_and_float32) {
    const std::vector<ArrayRef> text = {Array::from_strings(kTexts), Array::from_strings({}), Array::from_strings({"123.456"})};
    CHECK((bits_of<double, uint64_t>(ScalarFunctions::cast(text, DataType::Float64)) ==
           std::vector<unsigned long long>{0x40091eb851eb851full, 0x40f86a0000000000ull, 0x3fe0000000000000ull, 0x4014000000000000ull, 0x8000000000000000ull, 0x7ff8000000000000ull,
                                           0xfff0000000000000ull, 0x7ff0000000000000ull, 0xdeadull, 0xdeadull, 0xdeadull, 0x4340000000000000ull, 0x4340000000000001ull, 0x1ull,
                                           0x405edd2f1a9fbe77ull}));
    CHECK((bits_of<float, uint32_t>(ScalarFunctions::cast(text, DataType::Float32)) ==
           std::vector<unsigned long long>{0x4048f5c3, 0x47c35000, 0x3f000000, 0x40a00000, 0x80000000, 0x7fc00000, 0xff800000, 0x7f800000, 0xdeadull, 0xdeadull, 0xdeadull, 0x5a000000,
                                           0x5a000000, 0x0, 0x42f6e979}));
}

TEST(cast_floats_to_text) {
    const std::vector<bool> valid = {true, true, false, true, true, true, true, true, true, true, true, true};
    const std::vector<ArrayRef> doubles = {Array::from_vec<double>({1.0, 123.456, 7.0, 0.001, 9999999.999999998, 1e7, 1e23, f64_of(1), -0.0, f64_of(0x7ff0000000000000ull),
                                                                    f64_of(0x7ff8000000000001ull), 0.1 + 0.2}, &valid)};
    CHECK(strings_of(ScalarFunctions::cast(doubles, DataType::Utf8)) ==
          (std::vector<std::string>{"1.0", "123.456", "<null>", "0.001", "9999999.999999998", "1.0E7", "1.0E23", "4.9E-324", "-0.0", "Infinity", "NaN", "0.30000000000000004"}));
    const std::vector<ArrayRef> floats = {Array::from_vec<float>({1.0f, 0.1f, 3.4028235e38f, f32_of(1), 16777216.0f, -2.5f})};
    CHECK(strings_of(ScalarFunctions::cast(floats, DataType::Utf8)) == (std::vector<std::string>{"1.0", "0.1", "3.4028235E38", "1.4E-45", "1.6777216E7", "-2.5"}));
    // the round trip through the mirror
    CHECK((bits_of<float, uint32_t>(ScalarFunctions::cast(ScalarFunctions::cast(floats, DataType::Utf8), DataType::Float32)) == bits_of<float, uint32_t>(floats)));
}

TEST(column_methods) {
    const Column text = Column::from_arrays({Array::from_strings({"2.50", "x", "1e-3"})}, Field{"price", DataType::Utf8, false});
    const Column vals = text.utf8_parse_float(DataType::Float64);
    CHECK((bits_of<double, uint64_t>(vals.data().chunks()) == std::vector<unsigned long long>{0x4004000000000000ull, 0xdeadull, 0x3f50624dd2f1a9fcull}));
    CHECK(strings_of(vals.utf8_format_float().data().chunks()) == (std::vector<std::string>{"2.5", "<null>", "0.001"}));
    CHECK(strings_of(vals.cast_text(DataType::Utf8).data().chunks()) == (std::vector<std::string>{"2.5", "<null>", "0.001"}));
    CHECK((bits_of<float, uint32_t>(text.cast_text(DataType::Float32).data().chunks()) == std::vector<unsigned long long>{0x40200000, 0xdeadull, 0x3a83126f}));
    bool refused = false;
    try { vals.utf8_parse_float(DataType::Float64); } catch (const DataFrameError&) { refused = true; }   // not a text column
    CHECK(refused);
}

int main() { return run_all(); }
