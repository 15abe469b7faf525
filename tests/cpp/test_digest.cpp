// Row hashes and digests in the C++ mirror (rdf_frame.hpp -> rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32), on the
// device: Spark's documented answers through ScalarFunctions and the Column methods, NULL rows, and a hash of a text column
// as a GROUP BY key over uk_cities_with_headers.csv.
#include <map>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using SF = ScalarFunctions;
namespace P = plan;

static std::string g_csv = "tests/golden/uk_cities_with_headers.csv";

static std::vector<std::string> strings_of(const std::vector<ArrayRef>& chunks) {
    std::vector<std::string> out;
    for (auto& a : chunks)
        for (int64_t r = 0; r < a->length; ++r) out.push_back((*a->strings)[(size_t)(a->offset + r)]);
    return out;
}
template <class T> static std::vector<T> values_of(const std::vector<ArrayRef>& chunks) {
    std::vector<T> out;
    for (auto& a : chunks) { const auto v = a->values_to_host<T>(); out.insert(out.end(), v.begin(), v.end()); }
    return out;
}
static std::vector<std::string> S(std::initializer_list<const char*> v) { return std::vector<std::string>(v.begin(), v.end()); }

TEST(spark_known_answers) {
    const std::vector<ArrayRef> s = {Array::from_strings(S({"Spark"})), Array::from_strings(S({"", "Spark"}))};
    const std::vector<ArrayRef> a = {Array::from_vec(std::vector<int32_t>{123}), Array::from_vec(std::vector<int32_t>{7, 123})};
    const std::vector<ArrayRef> b = {Array::from_vec(std::vector<int32_t>{2}), Array::from_vec(std::vector<int32_t>{7, 2})};
    const std::vector<int32_t> h = values_of<int32_t>(SF::hash({s, a, b}));
    CHECK_EQ(h.size(), (size_t)3);
    CHECK_EQ(h[0], (int32_t)-1321691492);
    CHECK_EQ(h[2], (int32_t)-1321691492);
    CHECK(h[1] != h[0]);
    const std::vector<int64_t> x = values_of<int64_t>(SF::xxhash64({s, a, b}));
    CHECK_EQ(x[0], (int64_t)5602566077635097486LL);
    CHECK_EQ(x[2], (int64_t)5602566077635097486LL);
    CHECK(values_of<int32_t>(SF::hash({s, a, b}, 43))[0] != h[0]);
    CHECK_EQ(strings_of(SF::md5(s)), S({"8cde774d6f7333752ed72cacddb05126", "d41d8cd98f00b204e9800998ecf8427e", "8cde774d6f7333752ed72cacddb05126"}));
    CHECK_EQ(strings_of(SF::sha1(s))[0], std::string("85f5955f4b27a9a4c2aab6ffe5d7189fc298b92c"));
    CHECK_EQ(strings_of(SF::sha2(s, 256))[2], std::string("529bc3b07127ecb7e53a4dcf1991d9152c24537d919178022b2c42657f79a26b"));
    CHECK_EQ(strings_of(SF::sha2(s, 0)), strings_of(SF::sha2(s, 256)));
    CHECK_EQ(strings_of(SF::sha2(s, 224))[0].size(), (size_t)56);
    CHECK_EQ(strings_of(SF::sha2(s, 384))[0].size(), (size_t)96);
    CHECK_EQ(strings_of(SF::sha2(s, 512))[0].size(), (size_t)128);
    const std::vector<int64_t> crc = values_of<int64_t>(SF::crc32(s));
    CHECK_EQ(crc[0], (int64_t)1557323817);
    CHECK_EQ(crc[1], (int64_t)0);
    CHECK_THROWS(SF::sha2(s, 128));                                                // Spark returns NULL; here it is an error
    CHECK_THROWS(SF::md5({Array::from_vec(std::vector<int64_t>{1})}));              // Utf8 only
    CHECK_THROWS(SF::crc32({Array::from_vec(std::vector<int64_t>{1})}));
    CHECK_THROWS(SF::hash({s, std::vector<ArrayRef>{a[0]}}));                      // another chunking
    const Column cs = Column::from_arrays(s, Field{"s", DataType::Utf8, false});
    CHECK_EQ(strings_of(cs.md5().data().chunks()), strings_of(SF::md5(s)));
    CHECK_EQ(cs.sha1().data().num_chunks(), (size_t)2);
    CHECK_EQ(values_of<int32_t>(cs.hash().data().chunks()), values_of<int32_t>(SF::hash({s})));
    CHECK_EQ(values_of<int64_t>(cs.xxhash64().data().chunks()), values_of<int64_t>(SF::xxhash64({s})));
    const Column ci = Column::from_arrays(a, Field{"a", DataType::Int32, false});
    CHECK_EQ(values_of<int32_t>(ci.hash().data().chunks()), values_of<int32_t>(SF::hash({a})));
    CHECK_THROWS(ci.md5());
}

TEST(null_rows) {
    const Column src = Column::from_arrays({Array::from_strings(S({"Spark", "c"}))}, Field{"s", DataType::Utf8, false});
    const std::vector<bool> iv = {true, false, true};
    const Column t = src.take(Array::from_vec(std::vector<uint32_t>{0, 0, 1}, &iv), 1024);
    CHECK_EQ(t.data().chunk(0)->null_count, (int64_t)1);
    const Column m = t.md5();
    CHECK_EQ(strings_of(m.data().chunks()), S({"8cde774d6f7333752ed72cacddb05126", "", "4a8a08f09d37b73795649038408b5f33"}));
    CHECK_EQ(m.data().chunk(0)->null_count, (int64_t)1);
    CHECK_EQ(m.data().chunk(0)->valid_to_host(), iv);
    const Column c = t.crc32();
    CHECK_EQ(c.data().chunk(0)->null_count, (int64_t)1);
    CHECK_EQ(c.data().chunk(0)->valid_to_host(), iv);
    CHECK_EQ(values_of<int64_t>(c.data().chunks())[0], (int64_t)1557323817);
    // a NULL leaves the running hash alone: the seed comes back, and the result is never NULL
    const Column h = t.hash(42);
    CHECK(h.data().chunk(0)->validity == nullptr);
    CHECK_EQ(values_of<int32_t>(h.data().chunks())[1], (int32_t)42);
}

TEST(a_hash_is_a_group_by_key) {
    DataFrame base = DataFrame::from_csv(g_csv);
    std::vector<ArrayRef> milli;
    for (auto& a : base.column_by_name("lat").data().chunks()) {
        std::vector<int64_t> m;
        for (double x : a->values_to_host<double>()) m.push_back((int64_t)(x * 1000.0));
        milli.push_back(Array::from_vec(m));
    }
    base = base.with_column("milli", Column::from_arrays(milli, Field{"milli", DataType::Int64, false}));
    const Column region = base.column_by_name("city").lpad(1, "");             // a pad never lengthens past len: the city's first code point
    const Column key = Column::hash_columns(RDF_HASH_MURMUR3_32, {&region}, 42, "bucket");
    CHECK(key.data_type() == DataType::Int32);
    const DataFrame df = base.with_column("bucket", key);
    const std::vector<std::string> regions = strings_of(region.data().chunks());
    const std::vector<int32_t> buckets = values_of<int32_t>(df.column_by_name("bucket").data().chunks());
    const std::vector<int64_t> ms = values_of<int64_t>(df.column_by_name("milli").data().chunks());
    CHECK_EQ(buckets.size(), (size_t)37);
    std::map<std::string, int32_t> bucket_of;
    std::map<int32_t, std::pair<int64_t, int64_t>> want;
    for (size_t r = 0; r < regions.size(); ++r) {
        if (bucket_of.count(regions[r])) CHECK_EQ(bucket_of[regions[r]], buckets[r]);      // equal text, equal hash
        bucket_of[regions[r]] = buckets[r];
        want[buckets[r]].first += 1;
        want[buckets[r]].second += ms[r];
    }
    CHECK(want.size() > 2 && want.size() < 37);
    CHECK_EQ(want.size(), bucket_of.size());                                               // (no collision among these few)
    using AF = P::AggregateFunction;
    const DataFrame g = Evaluate::group_aggregate(df, {"bucket"}, {{AF::Count, {"milli"}}, {AF::Sum, {"milli"}}});
    CHECK_EQ((size_t)g.num_rows(), want.size());
    const std::vector<int32_t> gk = values_of<int32_t>(g.column(0).data().chunks());
    const std::vector<uint32_t> counts = values_of<uint32_t>(g.column_by_name("count(milli)").data().chunks());
    const std::vector<int64_t> sums = values_of<int64_t>(g.column_by_name("sum(milli)").data().chunks());
    size_t i = 0;
    for (auto& kv : want) {   // ordered by the grouping column
        CHECK_EQ(gk[i], kv.first);
        CHECK_EQ((int64_t)counts[i], kv.second.first);
        CHECK_EQ(sums[i], kv.second.second);
        ++i;
    }
}

int main() { return run_all(); }
