// Text keys in the C++ mirror (rdf_frame.hpp -> rdf_groupby_agg_keys / rdf_equijoin_indices_keys / rdf_utf8_dictionary_encode),
// run on the device over uk_cities_with_headers.csv: Evaluate::group_aggregate by a text column (alone and next to an integer one) against a
// std::map built here, a self-join on a text column, and Column::dictionary_encode followed by take of the dictionary.
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
namespace P = rdf::plan;

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

// the CSV plus: `initial` (Utf8, the city's first letter), `north` (Int64, 1 above 53 degrees), `milli` (Int64, lat in
// thousandths: sums of it are exact in any order) — all chunked like the frame
static DataFrame cities() {
    DataFrame df = DataFrame::from_csv(g_csv);
    std::vector<ArrayRef> ini, north, milli;
    const auto& lat_chunks = df.column_by_name("lat").data().chunks();
    size_t i = 0;
    for (auto& a : df.column(0).data().chunks()) {
        std::vector<std::string> s;
        for (int64_t r = 0; r < a->length; ++r) s.push_back((*a->strings)[(size_t)(a->offset + r)].substr(0, 1));
        ini.push_back(Array::from_strings(std::move(s)));
        const std::vector<double> lat = lat_chunks[i++]->values_to_host<double>();
        std::vector<int64_t> n, m;
        for (double x : lat) { n.push_back(x > 53.0 ? 1 : 0); m.push_back((int64_t)(x * 1000.0)); }
        north.push_back(Array::from_vec(n));
        milli.push_back(Array::from_vec(m));
    }
    return df.with_column("initial", Column::from_arrays(ini, Field{"initial", DataType::Utf8, false}))
        .with_column("north", Column::from_arrays(north, Field{"north", DataType::Int64, false}))
        .with_column("milli", Column::from_arrays(milli, Field{"milli", DataType::Int64, false}));
}

TEST(group_by_the_text_column_count_and_sum) {
    const DataFrame df = cities();
    CHECK_EQ(df.num_rows(), (int64_t)37);
    const std::vector<std::string> ini = strings_of(df.column_by_name("initial")), city = strings_of(df.column_by_name("city"));
    const std::vector<int64_t> milli = values_of<int64_t>(df.column_by_name("milli"));
    std::map<std::string, std::pair<int64_t, int64_t>> want;   // initial -> (rows, sum of milli); iterated in byte order
    for (size_t r = 0; r < ini.size(); ++r) { want[ini[r]].first += 1; want[ini[r]].second += milli[r]; }
    using AF = P::AggregateFunction;
    const DataFrame g = Evaluate::group_aggregate(df, {"initial"}, {{AF::Count, {"milli"}}, {AF::Sum, {"milli"}}});
    CHECK_EQ(g.num_columns(), (size_t)3);
    CHECK_EQ((size_t)g.num_rows(), want.size());
    CHECK(g.column(0).data_type() == DataType::Utf8);
    const std::vector<std::string> keys = strings_of(g.column(0));
    const std::vector<uint32_t> counts = values_of<uint32_t>(g.column_by_name("count(milli)"));
    const std::vector<int64_t> sums = values_of<int64_t>(g.column_by_name("sum(milli)"));
    size_t i = 0;
    for (auto& kv : want) {   // ordered by the grouping column, text in byte order
        CHECK_EQ(keys[i], kv.first);
        CHECK_EQ((int64_t)counts[i], kv.second.first);
        CHECK_EQ(sums[i], kv.second.second);
        ++i;
    }
    // the CSV's own text column: every city is a group of one row
    const DataFrame by_city = Evaluate::group_aggregate(df, {"city"}, {{AF::Count, {"lat"}}, {AF::Max, {"lat"}}});
    CHECK_EQ(by_city.num_rows(), (int64_t)37);
    std::map<std::string, double> lat_of;
    const std::vector<double> lat = values_of<double>(df.column_by_name("lat"));
    for (size_t r = 0; r < city.size(); ++r) lat_of[city[r]] = lat[r];
    const std::vector<std::string> ck = strings_of(by_city.column(0));
    const std::vector<double> mx = values_of<double>(by_city.column_by_name("max(lat)"));
    i = 0;
    for (auto& kv : lat_of) { CHECK_EQ(ck[i], kv.first); CHECK_EQ(mx[i], kv.second); ++i; }
}

TEST(group_by_a_text_and_an_integer_column) {
    const DataFrame df = cities();
    const std::vector<std::string> ini = strings_of(df.column_by_name("initial"));
    const std::vector<int64_t> north = values_of<int64_t>(df.column_by_name("north")), milli = values_of<int64_t>(df.column_by_name("milli"));
    std::map<std::pair<std::string, int64_t>, std::pair<int64_t, int64_t>> want;
    for (size_t r = 0; r < ini.size(); ++r) { auto& w = want[{ini[r], north[r]}]; w.first += 1; w.second += milli[r]; }
    using AF = P::AggregateFunction;
    const DataFrame g = Evaluate::group_aggregate(df, {"initial", "north"}, {{AF::Sum, {"milli"}}, {AF::Count, {"milli"}}});
    CHECK_EQ((size_t)g.num_rows(), want.size());
    const std::vector<std::string> k0 = strings_of(g.column(0));
    const std::vector<int64_t> k1 = values_of<int64_t>(g.column(1)), sums = values_of<int64_t>(g.column_by_name("sum(milli)"));
    const std::vector<uint32_t> counts = values_of<uint32_t>(g.column_by_name("count(milli)"));
    size_t i = 0;
    for (auto& kv : want) {
        CHECK_EQ(k0[i], kv.first.first);
        CHECK_EQ(k1[i], kv.first.second);
        CHECK_EQ((int64_t)counts[i], kv.second.first);
        CHECK_EQ(sums[i], kv.second.second);
        ++i;
    }
    // the other way round: the integer column leads the order
    const DataFrame h = Evaluate::group_aggregate(df, {"north", "initial"}, {{AF::Sum, {"milli"}}});
    CHECK_EQ((size_t)h.num_rows(), want.size());
    const std::vector<int64_t> h0 = values_of<int64_t>(h.column(0));
    for (size_t r = 1; r < h0.size(); ++r) CHECK(h0[r - 1] <= h0[r]);
    // integer columns only: the plan's GroupAggregate step, same answer either way
    const DataFrame n1 = Evaluate::group_aggregate(df, {"north"}, {{AF::Sum, {"milli"}}});
    const DataFrame n2 = LazyFrame::read(df).aggregate({"north"}, {{AF::Sum, {"milli"}}}).evaluate();
    CHECK(values_of<int64_t>(n1.column(0)) == values_of<int64_t>(n2.column(0)));
    CHECK(values_of<int64_t>(n1.column(1)) == values_of<int64_t>(n2.column(1)));
    CHECK_THROWS(Evaluate::group_aggregate(df, {"lat"}, {{AF::Sum, {"milli"}}}));   // a Float64 grouping column
}

TEST(self_join_on_the_text_column) {
    const DataFrame df = cities();
    const std::vector<std::string> ini = strings_of(df.column_by_name("initial")), city = strings_of(df.column_by_name("city"));
    const DataFrame right = DataFrame::from_columns({df.column_by_name("initial").renamed("r_initial"), df.column_by_name("city").renamed("r_city"),
                                                     df.column_by_name("milli").renamed("r_milli")});
    // probe rows ascending, partners ascending: the expected pairs in order
    std::vector<std::pair<size_t, size_t>> want;
    for (size_t l = 0; l < ini.size(); ++l)
        for (size_t r = 0; r < ini.size(); ++r) if (ini[l] == ini[r]) want.push_back({l, r});
    const DataFrame j = df.join(right, {DataFrame::JoinType::InnerJoin, {{"initial", "r_initial"}}});
    CHECK_EQ((size_t)j.num_rows(), want.size());
    CHECK(want.size() > 37);
    const std::vector<std::string> lc = strings_of(j.column_by_name("city")), rc = strings_of(j.column_by_name("r_city"));
    const std::vector<std::string> li = strings_of(j.column_by_name("initial")), ri = strings_of(j.column_by_name("r_initial"));
    const std::vector<int64_t> lm = values_of<int64_t>(j.column_by_name("milli")), rm = values_of<int64_t>(j.column_by_name("r_milli"));
    const std::vector<int64_t> milli = values_of<int64_t>(df.column_by_name("milli"));
    for (size_t p = 0; p < want.size(); ++p) {
        CHECK_EQ(lc[p], city[want[p].first]);
        CHECK_EQ(rc[p], city[want[p].second]);
        CHECK_EQ(li[p], ri[p]);
        CHECK_EQ(lm[p], milli[want[p].first]);
        CHECK_EQ(rm[p], milli[want[p].second]);
    }
    // every city is distinct: the join on the CSV's own text column is the identity; through the lazy frame as well
    const DataFrame id = df.join(right, {DataFrame::JoinType::FullJoin, {{"city", "r_city"}}});
    CHECK_EQ(id.num_rows(), (int64_t)37);
    CHECK(strings_of(id.column_by_name("city")) == strings_of(id.column_by_name("r_city")));
    const DataFrame lz = LazyFrame::read(df).join(LazyFrame::read(right), {DataFrame::JoinType::InnerJoin, {{"city", "r_city"}, {"milli", "r_milli"}}}).evaluate();
    CHECK_EQ(lz.num_rows(), (int64_t)37);
    CHECK(strings_of(lz.column_by_name("city")) == city);
    CHECK_THROWS(df.join(right, {DataFrame::JoinType::InnerJoin, {{"city", "r_milli"}}}));   // a text key pairs with a text key only
}

TEST(dictionary_encode_then_take_reproduces_the_column) {
    const DataFrame df = cities();
    for (const char* name : {"initial", "city"}) {
        const Column& col = df.column_by_name(name);
        const auto enc = col.dictionary_encode();
        const Column& codes = enc.first;
        const Column& dict = enc.second;
        CHECK(codes.data_type() == DataType::UInt32);
        CHECK(dict.data_type() == DataType::Utf8);
        CHECK_EQ(codes.data().num_chunks(), col.data().num_chunks());
        CHECK_EQ(codes.num_rows(), col.num_rows());
        // codes follow first occurrences: a new value's code is the number of distinct values seen before it
        const std::vector<uint32_t> c = values_of<uint32_t>(codes);
        const std::vector<std::string> rows = strings_of(col), d = strings_of(dict);
        std::map<std::string, uint32_t> seen;
        for (size_t r = 0; r < rows.size(); ++r) {
            auto it = seen.find(rows[r]);
            if (it == seen.end()) it = seen.emplace(rows[r], (uint32_t)seen.size()).first;
            CHECK_EQ(c[r], it->second);
        }
        CHECK_EQ(d.size(), seen.size());
        for (auto& kv : seen) CHECK_EQ(d[kv.second], kv.first);
        // take of the dictionary by the codes, chunk by chunk
        std::vector<std::string> back;
        for (auto& chunk : codes.data().chunks()) {
            const Column t = dict.take(chunk, 4096);
            const std::vector<std::string> s = strings_of(t);
            back.insert(back.end(), s.begin(), s.end());
        }
        CHECK(back == rows);
    }
    CHECK_THROWS(df.column_by_name("lat").dictionary_encode());
}

int main(int argc, char** argv) {
    if (argc > 1) g_csv = argv[1];
    return run_all();
}
