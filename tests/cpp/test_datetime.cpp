// ScalarFunctions::year .. date_diff in the C++ mirror (rdf_frame.hpp -> rdf_datetime_fields / rdf_datetime_trunc /
// rdf_date_shift / rdf_date_diff), run on the device over Array::from_vec columns.  The answers are Spark's documented
// examples, written as literals; dates are day numbers since 1970-01-01:
//   2008-02-20 13929   2009-01-12 14256   2009-01-31 14275   2009-07-30 14455   2009-07-31 14456   2015-01-14 16449
//   2015-01-20 16455   2015-03-02 16496   2015-03-05 16499   2016-01-31 16831   2016-02-29 16860   2016-04-09 16900
//   2016-08-31 17044   2016-09-30 17074   2019-02-28 17955   2019-03-28 17983   2019-07-01 18078   2019-07-29 18106
//   2019-08-04 18112
#include <string>
#include <vector>

#include "mini_test.hpp"
#include "rdf_frame.hpp"

using namespace rdf;
using SF = ScalarFunctions;

template <class T> static std::vector<T> host(const ArrayRef& a) { return a->values_to_host<T>(); }
static std::vector<ArrayRef> dates(const std::vector<int32_t>& d, const std::vector<bool>* valid = nullptr) { return {Array::from_vec<int32_t>(d, valid)}; }
static std::vector<int32_t> I(std::initializer_list<int32_t> v) { return std::vector<int32_t>(v); }

TEST(spark_examples_of_the_fields) {
    CHECK_EQ(host<int32_t>(SF::day_of_week(dates({14455}), RDF_TIME_DAY)[0]), I({5}));        // dayofweek('2009-07-30') = 5
    CHECK_EQ(host<int32_t>(SF::week_of_year(dates({13929}), RDF_TIME_DAY)[0]), I({8}));       // weekofyear('2008-02-20') = 8
    CHECK_EQ(host<int32_t>(SF::day_of_year(dates({16900}), RDF_TIME_DAY)[0]), I({100}));      // dayofyear('2016-04-09') = 100
    CHECK_EQ(host<int32_t>(SF::quarter(dates({17044}), RDF_TIME_DAY)[0]), I({3}));            // quarter('2016-08-31') = 3
    CHECK_EQ(host<int32_t>(SF::year(dates({17044, 0, -1}), RDF_TIME_DAY)[0]), I({2016, 1970, 1969}));
    CHECK_EQ(host<int32_t>(SF::month(dates({17044, 0, -1}), RDF_TIME_DAY)[0]), I({8, 1, 12}));
    CHECK_EQ(host<int32_t>(SF::day_of_month(dates({17044, 0, -1}), RDF_TIME_DAY)[0]), I({31, 1, 31}));
}

TEST(timestamps_in_every_unit) {
    const int64_t t = 16499ll * 86400 + 9 * 3600 + 32 * 60 + 5;                               // 2015-03-05T09:32:05
    const std::vector<bool> valid = {true, false, true};
    const std::vector<ArrayRef> s = {Array::from_vec<int64_t>({t, 7, -1}, &valid)};
    CHECK_EQ(host<int32_t>(SF::minute(s, RDF_TIME_SECOND)[0]), I({32, 0, 59}));               // (a NULL row holds 0)
    CHECK_EQ(host<int32_t>(SF::second(s, RDF_TIME_SECOND)[0]), I({5, 0, 59}));
    CHECK_EQ(host<int32_t>(SF::to_date(s, RDF_TIME_SECOND)[0]), I({16499, 0, -1}));
    CHECK_EQ(SF::year(s, RDF_TIME_SECOND)[0]->null_count, (int64_t)1);
    CHECK(SF::year(s, RDF_TIME_SECOND)[0]->valid_to_host() == valid);
    const std::vector<ArrayRef> ms = {Array::from_vec<int64_t>({t * 1000 + 359})}, ns = {Array::from_vec<int64_t>({t * 1000000000ll + 359000000})};
    CHECK_EQ(host<int32_t>(SF::second(ms, RDF_TIME_MILLISECOND)[0]), I({5}));                 // the fraction is dropped
    CHECK_EQ(host<int32_t>(SF::hour(ns, RDF_TIME_NANOSECOND)[0]), host<int32_t>(SF::datetime_field(ns, RDF_TIME_NANOSECOND, RDF_DT_HOUR)[0]));
    const auto f = SF::datetime_fields(ns, RDF_TIME_NANOSECOND, {RDF_DT_YEAR, RDF_DT_MONTH, RDF_DT_DAY_OF_MONTH, RDF_DT_HOUR, RDF_DT_MINUTE, RDF_DT_SECOND, RDF_DT_DAY_OF_WEEK, RDF_DT_DATE});
    CHECK_EQ(f.size(), (size_t)8);
    const int32_t want[8] = {2015, 3, 5, 9, 32, 5, 5, 16499};                                 // a Thursday: 5
    for (int i = 0; i < 8; ++i) CHECK_EQ(host<int32_t>(f[(size_t)i][0]), I({want[i]}));
    // date_trunc('WEEK', '2015-03-05T09:32:05.359') = 2015-03-02T00:00:00
    CHECK_EQ(host<int64_t>(SF::date_trunc(ms, RDF_TIME_MILLISECOND, RDF_TRUNC_WEEK)[0]), std::vector<int64_t>({16496ll * 86400000}));
    CHECK_EQ(host<int64_t>(SF::date_trunc(ms, RDF_TIME_MILLISECOND, RDF_TRUNC_MINUTE)[0]), std::vector<int64_t>({(t - 5) * 1000}));
}

TEST(spark_examples_of_trunc_and_date_math) {
    CHECK_EQ(host<int32_t>(SF::trunc(dates({18112}), RDF_TRUNC_WEEK)[0]), I({18106}));        // trunc('2019-08-04', 'week') = 2019-07-29
    CHECK_EQ(host<int32_t>(SF::trunc(dates({18112}), RDF_TRUNC_QUARTER)[0]), I({18078}));     // trunc('2019-08-04', 'quarter') = 2019-07-01
    CHECK_EQ(host<int32_t>(SF::last_day(dates({14256}), RDF_TIME_DAY)[0]), I({14275}));       // last_day('2009-01-12') = 2009-01-31
    CHECK_EQ(host<int32_t>(SF::next_day(dates({16449}), RDF_TIME_DAY, 3)[0]), I({16455}));    // next_day('2015-01-14', 'TU') = 2015-01-20
    CHECK_EQ(host<int32_t>(SF::add_months(dates({17044, 17955}), RDF_TIME_DAY, 1)[0]), I({17074, 17983}));   // 2016-08-31 -> 2016-09-30, 2019-02-28 -> 2019-03-28
    CHECK_EQ(host<int32_t>(SF::add_months(dates({16831}), RDF_TIME_DAY, 1)[0]), I({16860}));  // 2016-01-31 -> 2016-02-29
    CHECK_EQ(host<int32_t>(SF::date_diff(dates({14456}), RDF_TIME_DAY, dates({14455}), RDF_TIME_DAY)[0]), I({1}));   // datediff('2009-07-31', '2009-07-30') = 1
    CHECK_EQ(host<int32_t>(SF::date_add(dates({14455}), RDF_TIME_DAY, 1)[0]), I({14456}));
    CHECK_EQ(host<int32_t>(SF::date_sub(dates({14456}), RDF_TIME_DAY, 1)[0]), I({14455}));
}

TEST(column_amounts_and_their_nulls) {
    const std::vector<bool> kvalid = {true, true, false, true};
    const std::vector<ArrayRef> d = dates({14455, 14455, 14455, 16449}), k = {Array::from_vec<int32_t>({1, -1, 5, 30}, &kvalid)};
    const auto added = SF::date_add(d, RDF_TIME_DAY, k);
    CHECK_EQ(host<int32_t>(added[0]), I({14456, 14454, 0, 16479}));
    CHECK(added[0]->valid_to_host() == kvalid);
    CHECK_EQ(host<int32_t>(SF::date_sub(d, RDF_TIME_DAY, k)[0])[3], 16419);
    CHECK_EQ(host<int32_t>(SF::add_months(d, RDF_TIME_DAY, k)[0])[1], 14425);                 // 2009-06-30
    const auto next = SF::next_day(d, RDF_TIME_DAY, {Array::from_vec<int32_t>({5, 6, 0, 3})});   // Thursday -> a week later; a weekday of 0: NULL
    CHECK_EQ(host<int32_t>(next[0]), I({14462, 14456, 0, 16455}));
    CHECK(next[0]->valid_to_host() == std::vector<bool>({true, true, false, true}));
    CHECK_EQ(next[0]->null_count, (int64_t)1);
}

TEST(refusals) {
    CHECK_THROWS(SF::trunc(dates({1}), RDF_TRUNC_HOUR));                                      // finer than a day
    CHECK_THROWS(SF::next_day(dates({1}), RDF_TIME_DAY, 8));
    CHECK_THROWS(SF::year({Array::from_vec<double>({1.0})}, RDF_TIME_SECOND));
    CHECK_THROWS(SF::year({Array::from_vec<int64_t>({1})}, RDF_TIME_DAY));                    // Date32 is Int32
    CHECK_THROWS(SF::datetime_fields(dates({1}), RDF_TIME_DAY, {RDF_DT_YEAR, RDF_DT_YEAR}));
    CHECK_THROWS(SF::date_diff(dates({1, 2}), RDF_TIME_DAY, dates({1}), RDF_TIME_DAY));
}

int main() { return run_all(); }
