// GroupAggregate steps with several hash aggregations in the C++ mirror (rdf_frame.hpp -> ONE rdf_groupby_multi call and one
// sort of the groups), run on the device: a step with Sum, Min, Max, Avg and Count must equal, column for column — names,
// dtypes, validity, values —, what the same frame gives when each aggregation is run as a step of its own (the
// per-aggregation path over rdf_groupby_agg / rdf_groupby_agg_keys, which a step with one hash aggregation still takes).
// Integer keys (sparse, with NULLs), a text key, two key columns; more groups than the one-pass route holds (the step then
// falls back to the per-aggregation path) and a step that mixes in CountDistinct / First.  The Float64 values are
// integer-valued, so sums and averages are exact in any order and the comparison is bit for bit.
#include <cstring>
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
namespace P = rdf::plan;
using AF = P::AggregateFunction;

static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

// rows in chunks of 1024 / 1 / the rest: k (Int64, sparse, some NULL), k2 (Int32, 0..3), s (Utf8, some NULL and the empty
// string), a (Int64, some NULL; group 0 of k holds only NULLs), b (Float64, integer-valued), c (UInt64 around 2^63)
static DataFrame frame_of(int64_t n, int64_t groups) {
    uint64_t seed = 12345 + (uint64_t)groups;
    std::vector<int64_t> cuts = {0, std::min<int64_t>(1024, n), std::min<int64_t>(1025, n), n};
    std::vector<ArrayRef> k, k2, s, a, b, c;
    for (size_t p = 0; p + 1 < cuts.size(); ++p) {
        std::vector<int64_t> vk, va; std::vector<int32_t> vk2; std::vector<std::string> vs; std::vector<double> vb; std::vector<uint64_t> vc;
        std::vector<bool> ok_k, ok_a, ok_s;
        for (int64_t r = cuts[p]; r < cuts[p + 1]; ++r) {
            const int64_t g = (int64_t)(lcg(seed) % (uint64_t)groups);
            vk.push_back(g * 100003 - 7);
            ok_k.push_back(g % 11 != 3);
            vk2.push_back((int32_t)(lcg(seed) % 4));
            vs.push_back(g % 7 == 0 ? std::string() : "name-" + std::to_string(g % 23));
            ok_s.push_back(g % 23 != 5);
            va.push_back((int64_t)lcg(seed) - (1ll << 30));
            ok_a.push_back(g != 0 && lcg(seed) % 5 != 0);
            vb.push_back((double)((int64_t)(lcg(seed) % 4001) - 2000));
            vc.push_back((1ull << 63) - 50 + lcg(seed) % 100);
        }
        k.push_back(Array::from_vec(vk, &ok_k)); a.push_back(Array::from_vec(va, &ok_a));
        k2.push_back(Array::from_vec(vk2)); b.push_back(Array::from_vec(vb)); c.push_back(Array::from_vec(vc));
        auto sa = std::const_pointer_cast<Array>(Array::from_strings(std::move(vs)));
        const auto bits = pack_bits(ok_s);
        sa->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
        check(rdf_copy_h2d(sa->validity->data(), bits.data(), (int64_t)bits.size()));
        int64_t nulls = 0;
        for (bool v : ok_s) nulls += !v;
        sa->null_count = nulls;
        s.push_back(sa);
    }
    return DataFrame::from_columns({Column::from_arrays(k, Field{"k", DataType::Int64, true}), Column::from_arrays(k2, Field{"k2", DataType::Int32, false}),
                                    Column::from_arrays(s, Field{"s", DataType::Utf8, true}), Column::from_arrays(a, Field{"a", DataType::Int64, true}),
                                    Column::from_arrays(b, Field{"b", DataType::Float64, false}), Column::from_arrays(c, Field{"c", DataType::UInt64, false})});
}

template <class T> static void same_values(const Column& x, const Column& y) {
    std::vector<T> vx, vy;
    std::vector<bool> ox, oy;
    for (auto& ch : x.data().chunks()) { const auto v = ch->values_to_host<T>(); vx.insert(vx.end(), v.begin(), v.end()); const auto o = ch->valid_to_host(); for (int64_t r = 0; r < ch->length; ++r) ox.push_back(o.empty() || o[(size_t)r]); }
    for (auto& ch : y.data().chunks()) { const auto v = ch->values_to_host<T>(); vy.insert(vy.end(), v.begin(), v.end()); const auto o = ch->valid_to_host(); for (int64_t r = 0; r < ch->length; ++r) oy.push_back(o.empty() || o[(size_t)r]); }
    CHECK_EQ(vx.size(), vy.size());
    CHECK(ox == oy);
    size_t bad = 0;
    for (size_t r = 0; r < vx.size() && r < vy.size(); ++r) if (ox[r] && std::memcmp(&vx[r], &vy[r], sizeof(T)) != 0) ++bad;
    CHECK_EQ(bad, (size_t)0);
}

static void same_column(const Column& x, const Column& y) {
    CHECK_EQ(x.name(), y.name());
    CHECK(x.data_type() == y.data_type());
    CHECK_EQ(x.num_rows(), y.num_rows());
    if (x.data_type() == DataType::Utf8) {
        std::vector<std::string> sx, sy; std::vector<bool> ox, oy;
        for (auto& ch : x.data().chunks()) { const auto o = ch->valid_to_host(); for (int64_t r = 0; r < ch->length; ++r) { sx.push_back((*ch->strings)[(size_t)(ch->offset + r)]); ox.push_back(o.empty() || o[(size_t)r]); } }
        for (auto& ch : y.data().chunks()) { const auto o = ch->valid_to_host(); for (int64_t r = 0; r < ch->length; ++r) { sy.push_back((*ch->strings)[(size_t)(ch->offset + r)]); oy.push_back(o.empty() || o[(size_t)r]); } }
        CHECK(sx == sy);
        CHECK(ox == oy);
        return;
    }
    switch (x.data_type()) {
        case DataType::Int32: same_values<int32_t>(x, y); break;
        case DataType::UInt32: same_values<uint32_t>(x, y); break;
        case DataType::Int64: same_values<int64_t>(x, y); break;
        case DataType::UInt64: same_values<uint64_t>(x, y); break;
        case DataType::Float64: same_values<double>(x, y); break;
        default: CHECK(false); break;
    }
}

// the step at once against every aggregation as a step of its own
static void one_step_equals_single_steps(const DataFrame& df, const std::vector<std::string>& keys, const std::vector<P::Aggregation>& aggs) {
    const DataFrame all = Evaluate::group_aggregate(df, keys, aggs);
    size_t col = keys.size();
    for (auto& agg : aggs)
        for (auto& name : agg.columns) {
            const DataFrame one = Evaluate::group_aggregate(df, keys, {P::Aggregation{agg.function, {name}}});
            CHECK_EQ(one.num_columns(), keys.size() + 1);
            CHECK_EQ(one.num_rows(), all.num_rows());
            for (size_t k = 0; k < keys.size(); ++k) same_column(all.column(k), one.column(k));
            CHECK(col < all.num_columns());
            same_column(all.column(col), one.column(keys.size()));
            ++col;
        }
    CHECK_EQ(col, all.num_columns());
}

static const std::vector<P::Aggregation> kFive = {{AF::Sum, {"a", "b"}}, {AF::Min, {"a", "c"}}, {AF::Max, {"b", "c"}}, {AF::Avg, {"a", "b"}}, {AF::Count, {"a"}}};

TEST(integer_key_sum_min_max_avg_count) {
    one_step_equals_single_steps(frame_of(5000, 97), {"k"}, kFive);
}

TEST(text_key_sum_min_max_avg_count) {
    one_step_equals_single_steps(frame_of(5000, 97), {"s"}, kFive);
}

TEST(two_key_columns) {
    const DataFrame df = frame_of(5000, 97);
    one_step_equals_single_steps(df, {"k", "k2"}, kFive);
    one_step_equals_single_steps(df, {"k2", "s"}, {{AF::Sum, {"b"}}, {AF::Avg, {"b"}}, {AF::Max, {"a"}}});
}

TEST(more_groups_than_the_one_pass_route_holds) {
    CHECK(rdf_groupby_multi_capacity(5) < 3000);
    one_step_equals_single_steps(frame_of(9000, 3000), {"k"}, {{AF::Sum, {"a"}}, {AF::Min, {"a"}}, {AF::Max, {"b"}}, {AF::Avg, {"b"}}, {AF::Count, {"a"}}});
}

TEST(mixed_with_sorted_aggregates_and_small_shapes) {
    const DataFrame df = frame_of(3000, 41);
    one_step_equals_single_steps(df, {"k"}, {{AF::Sum, {"a"}}, {AF::CountDistinct, {"k2"}}, {AF::Max, {"b"}}, {AF::First, {"b"}}});
    one_step_equals_single_steps(df, {"k"}, {{AF::CountDistinct, {"k2"}}, {AF::Sum, {"a"}}, {AF::Avg, {"a"}}});
    one_step_equals_single_steps(frame_of(1, 1), {"k"}, {{AF::Sum, {"a"}}, {AF::Count, {"a"}}});
    one_step_equals_single_steps(frame_of(1, 1), {"s"}, {{AF::Sum, {"b"}}, {AF::Min, {"b"}}});
}

int main() { return run_all(); }
