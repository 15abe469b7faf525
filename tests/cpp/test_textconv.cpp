// test_textconv.cpp — text to values and back in the C++ mirror (include/rdf_frame.hpp): ScalarFunctions::to_date(arr, fmt) /
// to_timestamp / unix_timestamp / from_unix_time / date_format, cast to and from Utf8, and the matching Column methods, held to
// the known answers of the header's "text to values and back" section.  Needs a GPU.
#include <cstdio>
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
template <class T>
static std::vector<long long> values_of(const std::vector<ArrayRef>& chunks, long long null_value = -777) {
    std::vector<long long> out;
    for (auto& a : chunks) {
        const std::vector<T> v = a->values_to_host<T>();
        const std::vector<bool> ok = a->valid_to_host();
        for (size_t r = 0; r < v.size(); ++r) out.push_back(ok[r] ? (long long)v[r] : null_value);
    }
    return out;
}

TEST(unix_timestamp_and_to_date_with_a_pattern) {
    const std::vector<ArrayRef> text = {Array::from_strings({"2016-04-08", "2016-13-08", "2020-02-29"}), Array::from_strings({}), Array::from_strings({"1970-01-01"})};
    CHECK(values_of<int64_t>(ScalarFunctions::unix_timestamp(text, "yyyy-MM-dd")) == (std::vector<long long>{1460073600, -777, 1582934400, 0}));
    CHECK(values_of<int32_t>(ScalarFunctions::to_date(text, "yyyy-MM-dd")) == (std::vector<long long>{16899, -777, 18321, 0}));
    const std::vector<ArrayRef> stamps = {Array::from_strings({"2020-02-29T12:34:56.789", "2020-02-29 12:34:56.789"})};
    CHECK(values_of<int64_t>(ScalarFunctions::to_timestamp(stamps, RDF_TIME_MILLISECOND, "yyyy-MM-dd'T'HH:mm:ss.SSS")) == (std::vector<long long>{1582979696789, -777}));
}

TEST(date_format_and_from_unix_time) {
    const std::vector<ArrayRef> days = {Array::from_vec<int32_t>({18321, 0})};
    CHECK(strings_of(ScalarFunctions::date_format(days, RDF_TIME_DAY, "EEE, d MMM yyyy")) == (std::vector<std::string>{"Sat, 29 Feb 2020", "Thu, 1 Jan 1970"}));
    const std::vector<bool> valid = {true, false, true};
    const std::vector<ArrayRef> secs = {Array::from_vec<int64_t>({0, 5, 1460073600}, &valid)};
    CHECK(strings_of(ScalarFunctions::from_unix_time(secs, "yyyy-MM-dd HH:mm:ss")) == (std::vector<std::string>{"1970-01-01 00:00:00", "<null>", "2016-04-08 00:00:00"}));
}

TEST(cast_to_and_from_text) {
    const std::vector<ArrayRef> text = {Array::from_strings({" 42", "12.7", "-12.7", "128", "-128", "1e3", ""})};
    CHECK(values_of<int64_t>(ScalarFunctions::cast(text, DataType::Int64)) == (std::vector<long long>{42, 12, -12, 128, -128, -777, -777}));
    CHECK(values_of<int8_t>(ScalarFunctions::cast(text, DataType::Int8)) == (std::vector<long long>{42, 12, -12, -777, -128, -777, -777}));
    const std::vector<ArrayRef> ints = {Array::from_vec<int64_t>({0, -1, INT64_MIN, INT64_MAX})};
    CHECK(strings_of(ScalarFunctions::cast(ints, DataType::Utf8)) == (std::vector<std::string>{"0", "-1", "-9223372036854775808", "9223372036854775807"}));
    const std::vector<ArrayRef> flags = {Array::from_bools({true, false})};
    CHECK(strings_of(ScalarFunctions::cast(flags, DataType::Utf8)) == (std::vector<std::string>{"true", "false"}));
    const std::vector<ArrayRef> words = {Array::from_strings({"Yes", "n", "maybe"})};
    const auto back = ScalarFunctions::cast(words, DataType::Boolean);
    CHECK(back[0]->bools_to_host()[0] && !back[0]->bools_to_host()[1] && back[0]->is_null(2) && !back[0]->is_null(0));
    // the round trip through the mirror
    CHECK(values_of<int64_t>(ScalarFunctions::cast(ScalarFunctions::cast(ints, DataType::Utf8), DataType::Int64)) == (std::vector<long long>{0, -1, INT64_MIN, INT64_MAX}));
}

TEST(column_methods) {
    const Column text = Column::from_arrays({Array::from_strings({"08/04/16", "29/02/20"})}, Field{"when", DataType::Utf8, false});
    const Column days = text.to_date("dd/MM/yy");
    CHECK(values_of<int32_t>(days.data().chunks()) == (std::vector<long long>{16899, 18321}));
    CHECK(strings_of(days.date_format(RDF_TIME_DAY, "yyyy-MM-dd").data().chunks()) == (std::vector<std::string>{"2016-04-08", "2020-02-29"}));
    CHECK(values_of<int64_t>(text.unix_timestamp("dd/MM/yy").data().chunks()) == (std::vector<long long>{1460073600, 1582934400}));
    bool refused = false;
    try { text.to_date("yyy"); } catch (const DataFrameError&) { refused = true; }
    CHECK(refused);
}

int main() { return run_all(); }
