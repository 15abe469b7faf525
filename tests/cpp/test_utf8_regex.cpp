// Regular expressions in the C++ mirror (rdf_frame.hpp -> rdf_utf8_regexp_match / _count / _extract / _replace / _split), on the
// device: ScalarFunctions over chunk lists against results worked out by hand from java.util.regex's rules (leftmost-first,
// Matcher.find's resume rule, String.split), the Column methods over NULL rows and uk_cities_with_headers.csv, and
// DataFrame::filter with BooleanFilter::rlike alone and joined with a numeric comparison.
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using BF = BooleanFilter;
using SF = ScalarFunctions;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

static std::vector<std::string> strings_of(const Column& c) {
    std::vector<std::string> out;
    for (auto& a : c.data().chunks())
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
static std::vector<std::string> S(std::initializer_list<const char*> v) { return std::vector<std::string>(v.begin(), v.end()); }
static std::vector<int32_t> I(std::initializer_list<int32_t> v) { return std::vector<int32_t>(v); }
static std::vector<bool> B(std::initializer_list<bool> v) { return std::vector<bool>(v); }
static Column text(const std::vector<ArrayRef>& a) { return Column::from_arrays(a, Field{"c", DataType::Utf8, false}); }
static std::vector<int32_t> ints(const std::vector<ArrayRef>& r) { std::vector<int32_t> out; for (auto& a : r) for (auto v : a->values_to_host<int32_t>()) out.push_back(v); return out; }
static std::vector<bool> bools(const std::vector<ArrayRef>& r) { std::vector<bool> out; for (auto& a : r) for (bool v : a->bools_to_host()) out.push_back(v); return out; }

TEST(scalar_functions_over_chunk_lists) {
    const std::vector<ArrayRef> a = {Array::from_strings(S({"AB12 x", "baaac", "", "a中b ,  c,"})), Array::from_strings(S({"abab", "é\n😀"}))};
    CHECK(bools(SF::rlike(a, "^[A-Z]{2}\\d+")) == B({true, false, false, false, false, false}));
    CHECK(bools(SF::rlike(a, "a.b")) == B({false, false, false, true, false, false}));       // '.' takes the 3-byte character whole
    CHECK(bools(SF::rlike(a, "é.😀")) == B({false, false, false, false, false, false}));      // '.' does not match '\n'
    CHECK(bools(SF::rlike(a, "(?s)é.😀")) == B({false, false, false, false, false, true}));
    CHECK(bools(SF::rlike(a, "")) == B({true, true, true, true, true, true}));                // the empty pattern matches everywhere
    CHECK_EQ(SF::rlike(a, "a")[1]->dtype, DataType::Boolean);
    CHECK_EQ(ints(SF::regexp_count(a, "a")), I({0, 3, 0, 1, 2, 0}));
    CHECK_EQ(ints(SF::regexp_count(a, "a*")), I({7, 4, 1, 10, 5, 4}));                         // empty matches: at code points, not bytes
    CHECK_EQ(SF::regexp_count(a, "a")[0]->dtype, DataType::Int32);
    CHECK_EQ(strings_of(text(SF::regexp_extract(a, "a|ab"))), S({"", "a", "", "a", "a", ""}));         // leftmost-first, not longest
    CHECK_EQ(strings_of(text(SF::regexp_extract(a, "ab|a", 0))), S({"", "a", "", "a", "ab", ""}));
    CHECK_EQ(strings_of(text(SF::regexp_extract(a, "\\d+"))), S({"12", "", "", "", "", ""}));
    CHECK_EQ(strings_of(text(SF::regexp_replace(a, "a*", "-"))), S({"-A-B-1-2- -x-", "-b--c-", "-", "--中-b- -,- - -c-,-", "--b--b-", "-é-\n-😀-"}));
    CHECK_EQ(strings_of(text(SF::regexp_replace(a, "[^0-9]", ""))), S({"12", "", "", "", "", ""}));
    CHECK_EQ(strings_of(text(SF::regexp_replace(a, "\\s+", " "))), S({"AB12 x", "baaac", "", "a中b , c,", "abab", "é 😀"}));
    CHECK_EQ(strings_of(text(SF::regexp_replace(a, "^a", "\\$"))), S({"AB12 x", "baaac", "", "$中b ,  c,", "$bab", "é\n😀"}));   // '^' fails on resume
    CHECK_EQ(text(a).regexp_replace("a", "b").data().num_chunks(), (size_t)2);
    const ListArray l = SF::split_regexp(a, "\\s*,\\s*");
    CHECK_EQ(l.len(), (int64_t)6);
    CHECK(l.value_type() == DataType::Utf8);
    CHECK_EQ(l.value_offsets(), (std::vector<int32_t>{0, 1, 2, 3, 6, 7, 8}));
    CHECK_EQ(*l.child->strings, S({"AB12 x", "baaac", "", "a中b", "c", "", "abab", "é\n😀"}));   // trailing empty strings are kept
    CHECK_EQ(SF::split_regexp(a, "\\s*,\\s*", 2).value_offsets(), (std::vector<int32_t>{0, 1, 2, 3, 5, 6, 7}));
    CHECK_EQ(*SF::split_regexp(a, "\\s*,\\s*", 2).child->strings, S({"AB12 x", "baaac", "", "a中b", "c,", "abab", "é\n😀"}));
    // the Javadoc's own rows
    const std::vector<ArrayRef> boo = {Array::from_strings(S({"boo:and:foo", "abc"}))};
    CHECK_EQ(*SF::split_regexp(boo, "o", -1).child->strings, S({"b", "", ":and:f", "", "", "abc"}));
    CHECK_EQ(*SF::split_regexp(boo, ":", 2).child->strings, S({"boo", "and:foo", "abc"}));
    CHECK_EQ(*SF::split_regexp(boo, "", -1).child->strings, S({"b", "o", "o", ":", "a", "n", "d", ":", "f", "o", "o", "", "a", "b", "c", ""}));
}

TEST(refusals_throw_before_any_device_work) {
    const std::vector<ArrayRef> a = {Array::from_strings(S({"abc"}))};
    CHECK_THROWS(SF::rlike(a, "(a)\\1"));                       // a backreference
    CHECK_THROWS(SF::regexp_count(a, "\\bfoo"));                // \b
    CHECK_THROWS(SF::regexp_extract(a, "(a)", 1));              // capture groups are not built
    CHECK_THROWS(SF::regexp_replace(a, "a", "$1"));             // an unescaped '$'
    CHECK_THROWS(SF::regexp_replace(a, "a", "x\\"));            // a trailing backslash
    CHECK_THROWS(SF::split_regexp(a, "a{2,1}"));
    CHECK_THROWS(SF::rlike({Array::from_vec(std::vector<int64_t>{1})}, "a"));   // Utf8 only
}

TEST(null_rows) {
    const Column src = Column::from_arrays({Array::from_strings(S({"a-b", "c"}))}, Field{"s", DataType::Utf8, false});
    const std::vector<bool> iv = {true, false, true};
    const Column t = src.take(Array::from_vec(std::vector<uint32_t>{0, 0, 1}, &iv), 1024);
    CHECK_EQ(t.rlike("-").data().chunk(0)->null_count, (int64_t)1);
    CHECK_EQ(t.rlike("-").data().chunk(0)->valid_to_host(), iv);
    CHECK_EQ(t.regexp_count("[a-c]").data().chunk(0)->null_count, (int64_t)1);
    CHECK_EQ(strings_of(t.regexp_replace("[^a-z]", "")), S({"ab", "", "c"}));
    CHECK_EQ(t.regexp_replace("[^a-z]", "").data().chunk(0)->valid_to_host(), iv);
    CHECK_EQ(strings_of(t.regexp_extract("[bc]")), S({"b", "", "c"}));
    CHECK_EQ(t.regexp_extract("[bc]").data().chunk(0)->null_count, (int64_t)1);
    const ListArray l = t.split_regexp("[-]");
    CHECK_EQ(l.value_offsets(), (std::vector<int32_t>{0, 2, 2, 3}));
    CHECK(!l.is_null(0) && l.is_null(1) && !l.is_null(2));
}

TEST(filter_with_rlike) {
    const DataFrame df = DataFrame::from_csv(g_csv);
    const std::vector<std::string> city = strings_of(df.column_by_name("city"));
    // ^S : the six the LIKE 'S%' test counts; joined with a numeric comparison the three north of 52
    const auto rl = BF::rlike(BF::column("city"), BF::scalar("^S"));
    CHECK_EQ(df.filter(rl).num_rows(), (int64_t)6);
    CHECK_EQ(strings_of(df.filter(rl).column_by_name("city")), strings_of(df.filter(BF::like(BF::column("city"), BF::scalar("S%"))).column_by_name("city")));
    const DataFrame north = df.filter(BF::and_(rl, BF::gt(BF::column("lat"), BF::scalar(Scalar(52.0)))));
    CHECK_EQ(strings_of(north.column_by_name("city")), S({"Stoke-on-Trent, Staffordshire, the UK", "Solihull, Birmingham, UK", "Sutton Coldfield, West Midlands, UK"}));
    CHECK_EQ(north.num_columns(), df.num_columns());
    CHECK_EQ(strings_of(df.filter(BF::rlike(BF::column("city"), BF::scalar(", the UK$"))).column_by_name("city")),
             S({"Elgin, Scotland, the UK", "Stoke-on-Trent, Staffordshire, the UK", "Inverness, the UK"}));
    CHECK_EQ(strings_of(df.filter(BF::rlike(BF::column("city"), BF::scalar("(?i)^lONDON(?:derry)?,"))).column_by_name("city")), S({"London, UK", "Londonderry, Derry, UK"}));
    CHECK_EQ(df.filter(BF::not_(BF::rlike(BF::column("city"), BF::scalar("UK$")))).num_rows(), (int64_t)0);
    // a model on the host for one pattern: a city with a hyphen between two letters
    size_t want = 0;
    for (auto& c : city)
        for (size_t i = 1; i + 1 < c.size(); ++i)
            if (c[i] == '-' && std::isalpha((unsigned char)c[i - 1]) && std::isalpha((unsigned char)c[i + 1])) { ++want; break; }
    CHECK(want > 0);
    CHECK_EQ((size_t)df.filter(BF::rlike(BF::column("city"), BF::scalar("[A-Za-z]-[A-Za-z]"))).num_rows(), want);
    CHECK_THROWS(df.filter(BF::rlike(BF::column("city"), BF::scalar("(?=S)"))));              // look-ahead is refused
    CHECK_THROWS(df.filter(BF::rlike(BF::column("lat"), BF::scalar("5"))));                   // a numeric column
    CHECK_THROWS(df.filter(BF::rlike(BF::column("city"), BF::column("city"))));               // a pattern in a column
}

TEST(column_methods_over_the_csv) {
    const DataFrame base = DataFrame::from_csv(g_csv);
    const std::vector<std::string> city = strings_of(base.column_by_name("city"));
    // the country, whichever way the row spells it: everything up to the last ", " and an optional "the " removed
    const DataFrame df = base.with_column("country", base.column_by_name("city").regexp_replace("^.*, (?:the )?", ""));
    for (auto& c : strings_of(df.column_by_name("country"))) CHECK_EQ(c, std::string("UK"));
    // the first word
    const std::vector<std::string> first = strings_of(base.column_by_name("city").regexp_extract("^[^ ,]+"));
    for (size_t r = 0; r < city.size(); ++r) CHECK_EQ(first[r], city[r].substr(0, city[r].find_first_of(" ,")));
    // split at ", " written as a regular expression is split at the literal
    const ListArray re = base.column_by_name("city").split_regexp(",\\s"), lit = base.column_by_name("city").split(", ");
    CHECK_EQ(re.value_offsets(), lit.value_offsets());
    CHECK_EQ(*re.child->strings, *lit.child->strings);
    const DataFrame out = SF::explode(base, re, "part");
    CHECK_EQ(out.num_rows(), re.child->length);
    std::vector<int32_t> commas;
    for (auto& c : city) { int32_t k = 0; for (char ch : c) k += ch == ','; commas.push_back(k); }
    CHECK_EQ(ints(base.column_by_name("city").regexp_count(",").data().chunks()), commas);
}

int main() { return run_all(); }
