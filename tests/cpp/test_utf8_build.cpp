// The Utf8 builders in the C++ mirror (rdf_frame.hpp -> rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index), on the
// device over uk_cities_with_headers.csv: results go through DataFrame::with_column, a concatenated column is a GROUP BY key,
// a padded id is a sort key.
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using SF = ScalarFunctions;
namespace P = plan;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

static std::vector<std::string> strings_of(const Column& c) {
    std::vector<std::string> out;
    for (auto& a : c.data().chunks())
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
template <class T> static std::vector<T> values_of(const Column& c) {
    std::vector<T> out;
    for (auto& a : c.data().chunks()) { const auto v = a->values_to_host<T>(); out.insert(out.end(), v.begin(), v.end()); }
    return out;
}
static std::vector<std::string> S(std::initializer_list<const char*> v) { return std::vector<std::string>(v.begin(), v.end()); }

// the CSV plus `id` (Utf8: the row number), `region` (Utf8: what follows the last ", " of the city), `milli` (Int64)
static DataFrame cities() {
    DataFrame df = DataFrame::from_csv(g_csv);
    std::vector<ArrayRef> id, milli;
    int64_t row = 0;
    size_t i = 0;
    const auto& lat_chunks = df.column_by_name("lat").data().chunks();
    for (auto& a : df.column(0).data().chunks()) {
        std::vector<std::string> s;
        for (int64_t r = 0; r < a->length; ++r) s.push_back(std::to_string(row++ * 7 % 37));
        id.push_back(Array::from_strings(std::move(s)));
        std::vector<int64_t> m;
        for (double x : lat_chunks[i++]->values_to_host<double>()) m.push_back((int64_t)(x * 1000.0));
        milli.push_back(Array::from_vec(m));
    }
    return df.with_column("id", Column::from_arrays(id, Field{"id", DataType::Utf8, false}))
        .with_column("milli", Column::from_arrays(milli, Field{"milli", DataType::Int64, false}));
}

TEST(scalar_functions_over_chunk_lists) {
    const std::vector<ArrayRef> a = {Array::from_strings(S({"www.apache.org", "aaaa", "", "a中b"})), Array::from_strings(S({"x.y"}))};
    const std::vector<ArrayRef> b = {Array::from_strings(S({"1", "2", "3", "4"})), Array::from_strings(S({"5"}))};
    const Column ca = Column::from_arrays(a, Field{"a", DataType::Utf8, false});
    CHECK_EQ(strings_of(Column::from_arrays(SF::concat({a, ", ", b}), Field{"c", DataType::Utf8, false})), S({"www.apache.org, 1", "aaaa, 2", ", 3", "a中b, 4", "x.y, 5"}));
    CHECK_EQ(strings_of(Column::from_arrays(SF::concat_ws("-", {a, b, "z"}), Field{"c", DataType::Utf8, false})), S({"www.apache.org-1-z", "aaaa-2-z", "-3-z", "a中b-4-z", "x.y-5-z"}));
    CHECK_EQ(strings_of(Column::from_arrays(SF::lpad(b, 3, "0"), Field{"c", DataType::Utf8, false})), S({"001", "002", "003", "004", "005"}));
    CHECK_EQ(strings_of(Column::from_arrays(SF::rpad(a, 5, "é中"), Field{"c", DataType::Utf8, false})), S({"www.a", "aaaaé", "é中é中é", "a中bé中", "x.yé中"}));
    CHECK_EQ(strings_of(Column::from_arrays(SF::repeat(b, 3), Field{"c", DataType::Utf8, false})), S({"111", "222", "333", "444", "555"}));
    CHECK_EQ(strings_of(Column::from_arrays(SF::reverse(a), Field{"c", DataType::Utf8, false})), S({"gro.ehcapa.www", "aaaa", "", "b中a", "y.x"}));
    CHECK_EQ(strings_of(Column::from_arrays(SF::substring_index(a, ".", 2), Field{"c", DataType::Utf8, false})), S({"www.apache", "aaaa", "", "a中b", "x.y"}));
    CHECK_EQ(strings_of(ca.substring_index(".", -2)), S({"apache.org", "aaaa", "", "a中b", "x.y"}));
    CHECK_EQ(strings_of(ca.substring_index("aa", 2)), S({"www.apache.org", "a", "", "a中b", "x.y"}));
    CHECK_EQ(ca.reverse().data().num_chunks(), (size_t)2);
    CHECK_THROWS(SF::concat({"a", "b"}));                                   // no column part
    CHECK_THROWS(SF::concat({a, std::vector<ArrayRef>{b[0]}}));             // another chunking
    CHECK_THROWS(SF::lpad({Array::from_vec(std::vector<int64_t>{1})}, 3, "0"));   // Utf8 only
}

TEST(null_rows) {
    const auto valid = std::vector<bool>{true, false, true};
    // a NULL row made by take with a NULL index
    const Column src = Column::from_arrays({Array::from_strings(S({"ab", "c"}))}, Field{"s", DataType::Utf8, false});
    const std::vector<bool> iv = {true, false, true};
    const Column t = src.take(Array::from_vec(std::vector<uint32_t>{0, 0, 1}, &iv), 1024);
    CHECK_EQ(t.data().chunk(0)->null_count, (int64_t)1);
    const Column other = Column::from_arrays({Array::from_strings(S({"1", "2", "3"}))}, Field{"o", DataType::Utf8, false});
    const Column c = Column::concat({t, "-", other});
    CHECK_EQ(strings_of(c), S({"ab-1", "", "c-3"}));
    CHECK_EQ(c.data().chunk(0)->null_count, (int64_t)1);
    CHECK_EQ(c.data().chunk(0)->valid_to_host(), valid);
    const Column w = Column::concat_ws("-", {t, other});
    CHECK_EQ(strings_of(w), S({"ab-1", "2", "c-3"}));
    CHECK(w.data().chunk(0)->validity == nullptr);
    CHECK_EQ(t.lpad(4, "xy").data().chunk(0)->valid_to_host(), valid);
    CHECK_EQ(strings_of(t.lpad(4, "xy")), S({"xyab", "", "xyxc"}));
    CHECK_EQ(strings_of(t.repeat(2)), S({"abab", "", "cc"}));
}

TEST(a_concatenated_column_is_a_group_by_key) {
    const DataFrame base = cities();
    const Column region = base.column_by_name("city").substring_index(", ", -1);
    const Column initial = base.column_by_name("city").lpad(1, "");          // a pad never lengthens past len: the first code point
    const Column key = Column::concat_ws(" / ", {region, initial}, "key");
    const DataFrame df = base.with_column("key", key);
    CHECK_EQ(df.num_rows(), (int64_t)37);
    const std::vector<std::string> city = strings_of(df.column_by_name("city")), keys = strings_of(df.column_by_name("key"));
    const std::vector<int64_t> milli = values_of<int64_t>(df.column_by_name("milli"));
    std::map<std::string, std::pair<int64_t, int64_t>> want;
    for (size_t r = 0; r < city.size(); ++r) {
        const std::string reg = city[r].rfind(", ") == std::string::npos ? city[r] : city[r].substr(city[r].rfind(", ") + 2);
        const std::string k = reg + " / " + city[r].substr(0, 1);
        CHECK_EQ(keys[r], k);
        want[k].first += 1;
        want[k].second += milli[r];
    }
    CHECK(want.size() > 2 && want.size() < 37);
    using AF = P::AggregateFunction;
    const DataFrame g = Evaluate::group_aggregate(df, {"key"}, {{AF::Count, {"milli"}}, {AF::Sum, {"milli"}}});
    CHECK_EQ((size_t)g.num_rows(), want.size());
    const std::vector<std::string> gk = strings_of(g.column(0));
    const std::vector<uint32_t> counts = values_of<uint32_t>(g.column_by_name("count(milli)"));
    const std::vector<int64_t> sums = values_of<int64_t>(g.column_by_name("sum(milli)"));
    size_t i = 0;
    for (auto& kv : want) {   // ordered by the grouping column, text in byte order
        CHECK_EQ(gk[i], kv.first);
        CHECK_EQ((int64_t)counts[i], kv.second.first);
        CHECK_EQ(sums[i], kv.second.second);
        ++i;
    }
}

TEST(a_padded_id_sorts_like_its_number) {
    const DataFrame base = cities();
    const DataFrame df = base.with_column("padded", base.column_by_name("id").lpad(4, "0"));
    const std::vector<std::string> ids = strings_of(df.column_by_name("id")), padded = strings_of(df.column_by_name("padded"));
    for (size_t r = 0; r < ids.size(); ++r) CHECK_EQ(padded[r], std::string(4 - ids[r].size(), '0') + ids[r]);
    const DataFrame sorted = df.sort({{"padded", false, false}});
    const std::vector<std::string> got = strings_of(sorted.column_by_name("id"));
    CHECK_EQ(got.size(), (size_t)37);
    for (size_t r = 0; r < got.size(); ++r) CHECK_EQ(got[r], std::to_string(r));          // 7 r mod 37 is a permutation of 0 .. 36
    const std::vector<std::string> by_text = strings_of(df.sort({{"id", false, false}}).column_by_name("id"));
    CHECK(by_text != got);                                                                   // "10" sorts before "2" without the padding
    // the row travels with its key
    const std::vector<std::string> city = strings_of(df.column_by_name("city")), scity = strings_of(sorted.column_by_name("city"));
    for (size_t r = 0; r < ids.size(); ++r) CHECK_EQ(scity[(size_t)std::stoi(ids[r])], city[r]);
}

int main() { return run_all(); }
