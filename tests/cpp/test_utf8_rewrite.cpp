// The Utf8 rewrites in the C++ mirror (rdf_frame.hpp -> rdf_utf8_replace / _translate / _initcap / _split), on the device over
// uk_cities_with_headers.csv: initcap of the upper-cased city gives the title-cased names, split(city, ' ') explodes into one
// row per word, a replaced column is a GROUP BY key.  (The mirror has no upper(): the test upper-cases on the host.)
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
static Column text(const std::vector<ArrayRef>& a) { return Column::from_arrays(a, Field{"c", DataType::Utf8, false}); }

// ASCII title case by UTF8String.toTitleCase's word rule: the model of initcap for the CSV's names
static std::string title_ascii(std::string s) {
    bool word = true;
    for (char& c : s) {
        c = (char)(word ? std::toupper((unsigned char)c) : std::tolower((unsigned char)c));
        word = c == ' ';
    }
    return s;
}
static std::vector<std::string> split_host(const std::string& s, const std::string& d) {
    std::vector<std::string> out;
    size_t pos = 0;
    for (size_t h; (h = s.find(d, pos)) != std::string::npos; pos = h + d.size()) out.push_back(s.substr(pos, h - pos));
    out.push_back(s.substr(pos));
    return out;
}

TEST(scalar_functions_over_chunk_lists) {
    const std::vector<ArrayRef> a = {Array::from_strings(S({"sPark sql", "aaaaa", "", "a中b,c,"})), Array::from_strings(S({"ǄX  ßa\tb ΑΣ Σ"}))};
    CHECK_EQ(strings_of(text(SF::replace(a, "aa", "b"))), S({"sPark sql", "bba", "", "a中b,c,", "ǄX  ßa\tb ΑΣ Σ"}));
    CHECK_EQ(strings_of(text(SF::replace(a, "", "x"))), strings_of(text(a)));
    CHECK_EQ(strings_of(text(SF::replace(a, "中", ""))), S({"sPark sql", "aaaaa", "", "ab,c,", "ǄX  ßa\tb ΑΣ Σ"}));
    CHECK_EQ(strings_of(text(SF::translate(a, "a中,", "x-"))), S({"sPxrk sql", "xxxxx", "", "x-bc", "ǄX  ßx\tb ΑΣ Σ"}));
    CHECK_EQ(strings_of(text(SF::initcap(a))), S({"Spark Sql", "Aaaaa", "", "A中b,c,", "ǅx  ßa\tb Ας Σ"}));
    CHECK_EQ(text(a).initcap().data().num_chunks(), (size_t)2);
    const ListArray l = SF::split(a, ",", -1);
    CHECK_EQ(l.len(), (int64_t)5);
    CHECK_EQ(l.value_offsets(), (std::vector<int32_t>{0, 1, 2, 3, 6, 7}));
    CHECK(l.value_type() == DataType::Utf8);
    CHECK_EQ(*l.child->strings, S({"sPark sql", "aaaaa", "", "a中b", "c", "", "ǄX  ßa\tb ΑΣ Σ"}));
    CHECK_EQ(SF::split(a, ",", 2).value_offsets(), (std::vector<int32_t>{0, 1, 2, 3, 5, 6}));
    CHECK_THROWS(SF::split(a, "", -1));                                            // an empty delimiter
    CHECK_THROWS(SF::initcap({Array::from_vec(std::vector<int64_t>{1})}));         // Utf8 only
}

TEST(null_rows) {
    const Column src = Column::from_arrays({Array::from_strings(S({"a-b", "c"}))}, Field{"s", DataType::Utf8, false});
    const std::vector<bool> iv = {true, false, true};
    const Column t = src.take(Array::from_vec(std::vector<uint32_t>{0, 0, 1}, &iv), 1024);
    CHECK_EQ(strings_of(t.replace("-", "")), S({"ab", "", "c"}));
    CHECK_EQ(t.replace("-", "").data().chunk(0)->null_count, (int64_t)1);
    CHECK_EQ(t.initcap().data().chunk(0)->valid_to_host(), iv);
    CHECK_EQ(t.translate("ac", "x").data().chunk(0)->null_count, (int64_t)1);
    const ListArray l = t.split("-");
    CHECK_EQ(l.value_offsets(), (std::vector<int32_t>{0, 2, 2, 3}));
    CHECK(!l.is_null(0) && l.is_null(1) && !l.is_null(2));
}

TEST(initcap_of_the_upper_cased_city_is_its_title_case) {
    const DataFrame base = DataFrame::from_csv(g_csv);
    std::vector<ArrayRef> up;
    for (auto& a : base.column_by_name("city").data().chunks()) {
        std::vector<std::string> s;
        for (int64_t r = 0; r < a->length; ++r) {
            std::string x = (*a->strings)[(size_t)(a->offset + r)];
            std::transform(x.begin(), x.end(), x.begin(), [](unsigned char c) { return (char)std::toupper(c); });
            s.push_back(x);
        }
        up.push_back(Array::from_strings(std::move(s)));
    }
    const DataFrame df = base.with_column("title", Column::from_arrays(up, Field{"upper", DataType::Utf8, false}).initcap());
    const std::vector<std::string> city = strings_of(df.column_by_name("city")), title = strings_of(df.column_by_name("title"));
    CHECK_EQ(title.size(), (size_t)37);
    for (size_t r = 0; r < city.size(); ++r) CHECK_EQ(title[r], title_ascii(city[r]));
    CHECK_EQ(title[0], std::string("Elgin, Scotland, The Uk"));
}

TEST(split_city_into_words_and_explode) {
    const DataFrame base = DataFrame::from_csv(g_csv);
    const ListArray words = base.column_by_name("city").split(" ");
    CHECK_EQ(words.len(), (int64_t)37);
    const DataFrame out = SF::explode(base, words, "word");
    const std::vector<std::string> city = strings_of(base.column_by_name("city"));
    std::vector<std::string> want_word, want_city;
    for (auto& c : city)
        for (auto& w : split_host(c, " ")) { want_word.push_back(w); want_city.push_back(c); }
    CHECK_EQ((size_t)out.num_rows(), want_word.size());
    CHECK_EQ(strings_of(out.column_by_name("word")), want_word);
    CHECK_EQ(strings_of(out.column_by_name("city")), want_city);            // the row travels with its element
    CHECK_EQ(base.column_by_name("city").split(", ", 2).child->length, (int64_t)(2 * 37));   // every name has a ", "
}

TEST(a_replaced_column_is_a_group_by_key) {
    const DataFrame base = DataFrame::from_csv(g_csv);
    // "Elgin, Scotland, the UK" -> "the UK" -> "UK": the country, whichever way the row spells it
    const Column country = base.column_by_name("city").substring_index(", ", -1).replace("the ", "");
    std::vector<ArrayRef> one;
    for (auto& a : base.column(0).data().chunks()) one.push_back(Array::from_vec(std::vector<int64_t>((size_t)a->length, 1)));
    const DataFrame df = base.with_column("country", country).with_column("one", Column::from_arrays(one, Field{"one", DataType::Int64, false}));
    const std::vector<std::string> keys = strings_of(df.column_by_name("country"));
    std::map<std::string, int64_t> want;
    for (auto& k : keys) want[k] += 1;
    CHECK_EQ(want.size(), (size_t)1);
    CHECK_EQ(want["UK"], (int64_t)37);
    // and a key with more than one group: the first letter's case folded away by translate
    const Column initial = base.column_by_name("city").lpad(1, "").translate("ABCDEFGHIJKLMNOPQRSTUVWXYZ", "abcdefghijklmnopqrstuvwxyz");
    const DataFrame dg = df.with_column("initial", initial);
    std::map<std::string, int64_t> by_initial;
    for (auto& c : strings_of(base.column_by_name("city"))) by_initial[std::string(1, (char)std::tolower((unsigned char)c[0]))] += 1;
    using AF = P::AggregateFunction;
    const DataFrame g = Evaluate::group_aggregate(dg, {"initial"}, {{AF::Sum, {"one"}}});
    CHECK_EQ((size_t)g.num_rows(), by_initial.size());
    const std::vector<std::string> gk = strings_of(g.column(0));
    const std::vector<int64_t> sums = values_of<int64_t>(g.column_by_name("sum(one)"));
    size_t i = 0;
    for (auto& kv : by_initial) {   // ordered by the grouping column, text in byte order
        CHECK_EQ(gk[i], kv.first);
        CHECK_EQ(sums[i], kv.second);
        ++i;
    }
    const DataFrame gc = Evaluate::group_aggregate(df, {"country"}, {{AF::Sum, {"one"}}});
    CHECK_EQ(gc.num_rows(), (int64_t)1);
    CHECK_EQ(strings_of(gc.column(0)), S({"UK"}));
    CHECK_EQ(values_of<int64_t>(gc.column_by_name("sum(one)")), (std::vector<int64_t>{37}));
}

int main() { return run_all(); }
