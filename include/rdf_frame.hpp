// rdf_frame.hpp — C++17 host-side mirror of rust-dataframe's interface for the hot path, header-only
// over the C ABI of rdf_mi355x.h.  Columns live in HBM (RDF_MEM_DEVICE); every operation below is a
// call into librdf_mi355x.so — there is no host compute path here.
//
// Mirrors (paths relative to the reference root):
//   ChunkedArray / Column            src/table.rs:13-344        (from_arrays, slice, filter, take)
//   DataFrame                        src/dataframe.rs:30-337    (with_column, with_column_renamed, limit,
//                                                                filter, select, drop, to_record_batches)
//   Scalar / BooleanFilter           src/expression.rs:718-870  (eval_to_array)
//   Column / Calculation / Function / ScalarFunction / Transformation / Computation / Aggregation
//                                    src/expression.rs:286-712
//   Add/Subtract/Cast/Sin operations src/operation/scalar.rs:18-318 (plan builders: names, cast insertion)
//   Evaluate::{evaluate, calculate}  src/evaluation.rs:54-323
//   LazyFrame                        src/lazyframe.rs:15-315
//   AggregateFunctions               src/functions/aggregate.rs:12-93
// Where the reference materialises one DataFrame per plan step, Evaluate::evaluate here FUSES maximal
// runs of Calculate / Filter / aggregate steps into single passes over HBM (rdf_pipeline).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iterator>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <charconv>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "rdf_mi355x.h"

namespace rdf {

// ------------------------------------------------------------------------------------------------
// errors (src/error.rs:6-15)

struct DataFrameError : std::runtime_error {
    enum Kind { MemoryError, ParseError, ComputeError, DivideByZero, IoError, NoneError, ArrowError, SqlError, DeviceError } kind;
    DataFrameError(Kind k, const std::string& m) : std::runtime_error(m), kind(k) {}
};
inline void check(rdf_status s) {
    if (s == RDF_OK) return;
    const std::string msg = rdf_last_error();
    switch (s) {
        case RDF_COMPUTE_ERROR: throw DataFrameError(DataFrameError::ComputeError, msg);
        case RDF_DIVIDE_BY_ZERO: throw DataFrameError(DataFrameError::DivideByZero, msg);
        case RDF_INVALID_ARGUMENT: throw DataFrameError(DataFrameError::ArrowError, msg);
        case RDF_MEMORY_ERROR: throw DataFrameError(DataFrameError::MemoryError, msg);
        default: throw DataFrameError(DataFrameError::DeviceError, msg);
    }
}

// ------------------------------------------------------------------------------------------------
// data types

enum class DataType : int32_t {
    Int8 = RDF_I8, Int16 = RDF_I16, Int32 = RDF_I32, Int64 = RDF_I64, UInt8 = RDF_U8, UInt16 = RDF_U16,
    UInt32 = RDF_U32, UInt64 = RDF_U64, Float32 = RDF_F32, Float64 = RDF_F64, Boolean = RDF_BOOL, Utf8 = 100
};
inline const char* type_name(DataType t) {
    switch (t) {
        case DataType::Int8: return "Int8"; case DataType::Int16: return "Int16"; case DataType::Int32: return "Int32";
        case DataType::Int64: return "Int64"; case DataType::UInt8: return "UInt8"; case DataType::UInt16: return "UInt16";
        case DataType::UInt32: return "UInt32"; case DataType::UInt64: return "UInt64"; case DataType::Float32: return "Float32";
        case DataType::Float64: return "Float64"; case DataType::Boolean: return "Boolean"; default: return "Utf8";
    }
}
inline int type_size(DataType t) {
    switch (t) {
        case DataType::Int8: case DataType::UInt8: return 1;
        case DataType::Int16: case DataType::UInt16: return 2;
        case DataType::Int32: case DataType::UInt32: case DataType::Float32: return 4;
        case DataType::Int64: case DataType::UInt64: case DataType::Float64: return 8;
        default: return 0;
    }
}
inline bool is_integer(DataType t) { return (int)t <= RDF_U64; }
inline bool is_float(DataType t) { return t == DataType::Float32 || t == DataType::Float64; }
template <class T> struct TypeOf;
template <> struct TypeOf<int8_t> { static constexpr DataType value = DataType::Int8; };
template <> struct TypeOf<int16_t> { static constexpr DataType value = DataType::Int16; };
template <> struct TypeOf<int32_t> { static constexpr DataType value = DataType::Int32; };
template <> struct TypeOf<int64_t> { static constexpr DataType value = DataType::Int64; };
template <> struct TypeOf<uint8_t> { static constexpr DataType value = DataType::UInt8; };
template <> struct TypeOf<uint16_t> { static constexpr DataType value = DataType::UInt16; };
template <> struct TypeOf<uint32_t> { static constexpr DataType value = DataType::UInt32; };
template <> struct TypeOf<uint64_t> { static constexpr DataType value = DataType::UInt64; };
template <> struct TypeOf<float> { static constexpr DataType value = DataType::Float32; };
template <> struct TypeOf<double> { static constexpr DataType value = DataType::Float64; };

struct Field {
    std::string name;
    DataType data_type;
    bool nullable = true;
};
struct Schema {
    std::vector<Field> fields;
    std::optional<std::pair<size_t, Field>> column_with_name(const std::string& n) const {
        for (size_t i = 0; i < fields.size(); ++i) if (fields[i].name == n) return std::make_pair(i, fields[i]);
        return std::nullopt;
    }
};

// ------------------------------------------------------------------------------------------------
// device buffers and arrays (Arc<dyn Array> resident in HBM)

class DeviceBuffer {
  public:
    explicit DeviceBuffer(int64_t bytes) : bytes_(bytes) { check(rdf_dev_alloc(&ptr_, bytes + 64)); }
    // memory that belongs to something else (a frame the library returned): `keep` holds the owner alive
    DeviceBuffer(void* borrowed, int64_t bytes, std::shared_ptr<void> keep) : ptr_(borrowed), bytes_(bytes), keep_(std::move(keep)) {}
    ~DeviceBuffer() { if (ptr_ && !keep_) (void)rdf_dev_free(ptr_); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    void* data() const { return ptr_; }
    int64_t bytes() const { return bytes_; }
  private:
    void* ptr_ = nullptr;
    int64_t bytes_;
    std::shared_ptr<void> keep_;
};
using BufferRef = std::shared_ptr<DeviceBuffer>;

// Page-locked host memory (rdf_host_alloc): what a reader parses into / reads a file into, so that its uploads are plain DMA
// (no runtime staging copy) and can run on the copy stream while the reader goes on (rdf_copy_h2d_async ... rdf_copy_fence).
class PinnedBuffer {
  public:
    explicit PinnedBuffer(int64_t bytes) : bytes_(bytes) { check(rdf_host_alloc(&ptr_, bytes + 64)); }
    ~PinnedBuffer() { if (ptr_) (void)rdf_host_free(ptr_); }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    uint8_t* data() const { return (uint8_t*)ptr_; }
    int64_t bytes() const { return bytes_; }
  private:
    void* ptr_ = nullptr;
    int64_t bytes_;
};
// One load (from_csv / from_arrow): uploads from pinned memory are queued, ONE fence at the end.  `bytes` counts what went up.
struct IngestStats { int64_t bytes = 0, async_copies = 0, blocking_copies = 0; double seconds = 0, parse_seconds = 0; };
inline IngestStats& last_ingest() { static thread_local IngestStats s; return s; }
inline void upload(void* dst, const void* src, int64_t bytes, bool src_pinned) {
    if (bytes <= 0) return;
    IngestStats& st = last_ingest();
    st.bytes += bytes;
    if (src_pinned) { check(rdf_copy_h2d_async(dst, src, bytes)); ++st.async_copies; }
    else { check(rdf_copy_h2d(dst, src, bytes)); ++st.blocking_copies; }
}

// Uploads out of PAGEABLE memory (a file mapped into the address space): page-locking a whole multi-GB image costs more than moving
// it (hipHostMalloc of 2.57 GB: 0.44 s; the link moves it in 0.05 s), so the bytes go through two page-locked staging buffers of
// kGroup bytes that live as long as the thread: worker threads copy the pieces of one group out of the page cache while the
// copy stream drains the other.  Never pins more than 2 x kGroup, whatever the file's size.
class StagedUploader {
  public:
    static StagedUploader& instance() { static thread_local StagedUploader u; return u; }
    void push(void* dst, const void* src, int64_t bytes) {
        IngestStats& st = last_ingest();
        st.bytes += bytes > 0 ? bytes : 0;
        const uint8_t* p = (const uint8_t*)src;
        uint8_t* d = (uint8_t*)dst;
        while (bytes > 0) {
            if (!grp_[0]) { grp_[0] = std::make_unique<PinnedBuffer>(kGroup); grp_[1] = std::make_unique<PinnedBuffer>(kGroup); }
            const int64_t take = std::min(bytes, kGroup - used_);
            pieces_.push_back(Piece{d, p, take, used_});
            used_ += (take + 255) / 256 * 256;
            d += take; p += take; bytes -= take;
            if (used_ >= kGroup) flush();
        }
    }
    void flush() {      // the current group: pages -> staging buffer (threads), staging buffer -> HBM (queued on the copy stream)
        if (pieces_.empty()) return;
        uint8_t* base = grp_[cur_]->data();
        {   // long pieces are cut so that every thread has work: a group usually holds a few dozen column buffers
            std::vector<Piece> cut;
            for (const Piece& q : pieces_)
                for (int64_t o = 0; o < q.bytes; o += kSlice) cut.push_back(Piece{q.dst + o, q.src + o, std::min(kSlice, q.bytes - o), q.off + o});
            pieces_.swap(cut);
        }
        const int T = (int)std::max<size_t>(1, std::min<size_t>({pieces_.size(), (size_t)std::max(1u, std::thread::hardware_concurrency()), (size_t)12}));
        auto work = [&](int t) { for (size_t k = (size_t)t; k < pieces_.size(); k += (size_t)T) std::memcpy(base + pieces_[k].off, pieces_[k].src, (size_t)pieces_[k].bytes); };
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
        IngestStats& st = last_ingest();
        for (const Piece& q : pieces_) { check(rdf_copy_h2d_async(q.dst, base + q.off, q.bytes)); ++st.async_copies; }
        pieces_.clear();
        used_ = 0;
        inflight_[cur_] = true;
        cur_ ^= 1;
        if (inflight_[cur_]) { check(rdf_copy_fence()); inflight_[0] = inflight_[1] = false; }   // the buffer we turn to must have left
    }
    void finish() { flush(); check(rdf_copy_fence()); inflight_[0] = inflight_[1] = false; }
  private:
    struct Piece { uint8_t* dst; const uint8_t* src; int64_t bytes, off; };
    static constexpr int64_t kGroup = (int64_t)128 << 20, kSlice = (int64_t)4 << 20;
    std::unique_ptr<PinnedBuffer> grp_[2];
    std::vector<Piece> pieces_;
    int64_t used_ = 0;
    int cur_ = 0;
    bool inflight_[2] = {false, false};
};

inline std::vector<uint8_t> pack_bits(const std::vector<bool>& bits) {
    std::vector<uint8_t> out((bits.size() + 63) / 64 * 8 + 8, 0);
    for (size_t i = 0; i < bits.size(); ++i) if (bits[i]) out[i >> 3] |= (uint8_t)(1u << (i & 7));
    return out;
}

struct Array;
using ArrayRef = std::shared_ptr<const Array>;

struct Array {
    BufferRef values, validity;  // validity null = no nulls
    int64_t offset = 0, length = 0, null_count = 0;
    DataType dtype = DataType::Float64;
    std::shared_ptr<const std::vector<std::string>> strings;  // Utf8 columns are carried opaquely on the host
    // The buffers are HOST memory (DataFrame::from_arrow_host: views into the mapped file): the array can feed aggregates —
    // AggregateFunctions::*, a LazyFrame that ends in aggregate() — which the library then streams through HBM slab by slab
    // (rdf_pipeline over RDF_MEM_HOST, rdf_capi_stream.inc); operators that produce device columns want to_device() first.
    bool host = false;

    size_t len() const { return (size_t)length; }
    DataType data_type() const { return dtype; }

    rdf_array view() const {
        if (dtype == DataType::Utf8) throw DataFrameError(DataFrameError::ComputeError, "Utf8 arrays are not on the compute path");
        rdf_array a;
        a.values = values ? values->data() : nullptr;
        a.validity = validity ? (const uint8_t*)validity->data() : nullptr;
        a.offset = offset; a.length = length; a.null_count = null_count; a.dtype = (int32_t)dtype; a.mem = host ? RDF_MEM_HOST : RDF_MEM_DEVICE;
        return a;
    }
    rdf_array view_unknown_nulls() const { rdf_array a = view(); a.null_count = -1; return a; }
    rdf_out out_view(int64_t capacity) const {
        rdf_out o;
        o.values = values ? values->data() : nullptr;
        o.validity = validity ? (uint8_t*)validity->data() : nullptr;
        o.capacity = capacity; o.length = 0; o.null_count = 0; o.dtype = (int32_t)dtype; o.mem = host ? RDF_MEM_HOST : RDF_MEM_DEVICE;
        return o;
    }
    // freshly allocated output array (capacity rounded up to 64 elements as the ABI asks)
    // `on_host`: the output of an operator over a host-resident frame (DataFrame::from_arrow_host) lives in page-locked host
    // memory — the library streams such calls and its copies back are plain DMA into these buffers
    static std::shared_ptr<Array> make_out(DataType t, int64_t capacity, bool with_validity, bool on_host = false) {
        auto a = std::make_shared<Array>();
        const int64_t cap = (capacity + 63) / 64 * 64;
        a->dtype = t;
        a->host = on_host;
        auto buf = [&](int64_t bytes) -> BufferRef {
            if (!on_host) return std::make_shared<DeviceBuffer>(bytes);
            auto pin = std::make_shared<PinnedBuffer>(bytes);
            return std::make_shared<DeviceBuffer>(pin->data(), bytes, pin);
        };
        a->values = buf(t == DataType::Boolean ? cap / 8 + 8 : cap * type_size(t) + 8);
        if (with_validity) a->validity = buf(cap / 8 + 8);
        return a;
    }
    // bytes of this array's buffers on the caller's side of the link: a copy off the device, or straight out of host memory
    void fetch(void* dst, const void* src, int64_t bytes) const {
        if (bytes <= 0) return;
        if (host) std::memcpy(dst, src, (size_t)bytes);
        else check(rdf_copy_d2h(dst, src, bytes));
    }
    template <class T>
    static ArrayRef from_vec(const std::vector<T>& v, const std::vector<bool>* valid = nullptr) {
        auto a = std::make_shared<Array>();
        a->dtype = TypeOf<T>::value;
        a->length = (int64_t)v.size();
        a->values = std::make_shared<DeviceBuffer>((int64_t)(v.size() * sizeof(T)) + 8);
        if (!v.empty()) check(rdf_copy_h2d(a->values->data(), v.data(), (int64_t)(v.size() * sizeof(T))));
        if (valid) {
            const auto bits = pack_bits(*valid);
            a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
            check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
            for (bool b : *valid) a->null_count += !b;
        }
        return a;
    }
    static ArrayRef from_bools(const std::vector<bool>& v, const std::vector<bool>* valid = nullptr) {
        auto a = std::make_shared<Array>();
        a->dtype = DataType::Boolean;
        a->length = (int64_t)v.size();
        const auto bits = pack_bits(v);
        a->values = std::make_shared<DeviceBuffer>((int64_t)bits.size());
        check(rdf_copy_h2d(a->values->data(), bits.data(), (int64_t)bits.size()));
        if (valid) {
            const auto vb = pack_bits(*valid);
            a->validity = std::make_shared<DeviceBuffer>((int64_t)vb.size());
            check(rdf_copy_h2d(a->validity->data(), vb.data(), (int64_t)vb.size()));
            for (bool b : *valid) a->null_count += !b;
        }
        return a;
    }
    static ArrayRef from_strings(std::vector<std::string> s) {
        auto a = std::make_shared<Array>();
        a->dtype = DataType::Utf8;
        a->length = (int64_t)s.size();
        a->strings = std::make_shared<const std::vector<std::string>>(std::move(s));
        return a;
    }
    // Array::slice: zero-copy (src/table.rs:88)
    ArrayRef slice(int64_t off, int64_t len) const {
        auto a = std::make_shared<Array>(*this);
        if (off > length) off = length;
        if (len > length - off) len = length - off;
        a->offset = offset + off;
        a->length = len;
        a->null_count = validity ? -1 : 0;
        return a;
    }
    std::vector<bool> bits_to_host(const BufferRef& buf) const {
        std::vector<bool> out((size_t)length, true);
        if (!buf || length == 0) return out;
        const int64_t b0 = offset >> 3, b1 = (offset + length + 7) >> 3;
        std::vector<uint8_t> raw((size_t)(b1 - b0));
        fetch(raw.data(), (const uint8_t*)buf->data() + b0, b1 - b0);
        for (int64_t i = 0; i < length; ++i) { const int64_t k = (offset & 7) + i; out[(size_t)i] = (raw[(size_t)(k >> 3)] >> (k & 7)) & 1; }
        return out;
    }
    std::vector<bool> valid_to_host() const { return bits_to_host(validity); }
    std::vector<bool> bools_to_host() const { return bits_to_host(values); }
    template <class T>
    std::vector<T> values_to_host() const {
        if (TypeOf<T>::value != dtype) throw DataFrameError(DataFrameError::ComputeError, "values_to_host: type mismatch");
        std::vector<T> out((size_t)length);
        if (length) fetch(out.data(), (const T*)values->data() + offset, length * (int64_t)sizeof(T));
        return out;
    }
    bool is_null(int64_t i) const { return validity && !valid_to_host()[(size_t)i]; }
    template <class T> T value(int64_t i) const {
        T v;
        fetch(&v, (const T*)values->data() + offset + i, (int64_t)sizeof(T));
        return v;
    }
    int64_t count_nulls() const {  // resolves an unknown null_count on the device
        if (!validity) return 0;
        if (null_count >= 0) return null_count;
        rdf_array v = view();
        int64_t c = 0; int32_t some = 0;
        check(rdf_count(&v, 1, &c, &some));
        return length - c;
    }
};

inline std::vector<ArrayRef> cast_arrays(const std::vector<ArrayRef>& arr, DataType to);   // arrow::compute::cast per chunk, below

// ------------------------------------------------------------------------------------------------
// ChunkedArray (src/table.rs:13-112)

class ChunkedArray {
  public:
    ChunkedArray() = default;
    static ChunkedArray from_arrays(std::vector<ArrayRef> arrays) {
        if (arrays.empty()) throw DataFrameError(DataFrameError::ComputeError, "ChunkedArray needs at least 1 array");  // assert!, :25
        ChunkedArray c;
        for (auto& a : arrays) {
            if (a->dtype != arrays[0]->dtype) throw DataFrameError(DataFrameError::ComputeError, "arrays of a ChunkedArray share one data type");
            c.num_rows_ += a->length;
        }
        c.chunks_ = std::move(arrays);
        return c;
    }
    int64_t num_rows() const { return num_rows_; }
    int64_t null_count() const { int64_t n = 0; for (auto& a : chunks_) n += a->count_nulls(); return n; }
    size_t num_chunks() const { return chunks_.size(); }
    const ArrayRef& chunk(size_t i) const { return chunks_[i]; }
    const std::vector<ArrayRef>& chunks() const { return chunks_; }
    DataType data_type() const { return chunks_[0]->dtype; }
    std::vector<int64_t> chunk_counts() const { std::vector<int64_t> v; for (auto& a : chunks_) v.push_back(a->length); return v; }

    // zero-copy slice, src/table.rs:77-95 (same chunk walk)
    ChunkedArray slice(int64_t offset, std::optional<int64_t> length = std::nullopt) const {
        int64_t len = std::min(length.value_or(INT64_MAX), num_rows_);
        size_t cur = 0;
        std::vector<ArrayRef> out;
        while (cur < chunks_.size() && offset >= chunks_[cur]->length) { offset -= chunks_[cur]->length; ++cur; }
        while (cur < chunks_.size() && len > 0) {
            out.push_back(chunks_[cur]->slice(offset, len));
            len -= std::min(len, chunks_[cur]->length - offset);
            offset = 0;
            ++cur;
        }
        if (out.empty()) out.push_back(chunks_[0]->slice(0, 0));
        return from_arrays(std::move(out));
    }

    std::vector<rdf_array> views() const { std::vector<rdf_array> v; for (auto& a : chunks_) v.push_back(a->view()); return v; }

    // src/table.rs:97-107: zip(chunks, condition chunks) -> arrow::compute::filter
    ChunkedArray filter(const ChunkedArray& condition) const {
        if (condition.num_chunks() != num_chunks()) throw DataFrameError(DataFrameError::ComputeError, "filter: chunk counts differ");
        const auto cv = views(), mv = condition.views();
        std::vector<int64_t> counts(cv.size());
        check(rdf_filter_count(mv.data(), (int64_t)mv.size(), counts.data()));
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t i = 0; i < cv.size(); ++i) {
            outs.push_back(Array::make_out(data_type(), counts[i], chunks_[i]->validity != nullptr));
            ov.push_back(outs.back()->out_view(counts[i]));
        }
        check(rdf_filter(cv.data(), mv.data(), (int64_t)cv.size(), ov.data()));
        std::vector<ArrayRef> res;
        for (size_t i = 0; i < outs.size(); ++i) { outs[i]->length = ov[i].length; outs[i]->null_count = ov[i].null_count; res.push_back(outs[i]); }
        return from_arrays(std::move(res));
    }

  private:
    std::vector<ArrayRef> chunks_;
    int64_t num_rows_ = 0;
};

// ------------------------------------------------------------------------------------------------
// Column::hist / Column::uniques results (src/table.rs:140-158, 244-341)

// histo_fp::Histogram as the reference reads it back: buckets with start() / end() / count().  The buckets are
// numpy.histogram's over [min, max] (rdf_hist); with `density` a bucket also carries count / counted rows.
class Histogram {
  public:
    struct Bucket {
        double start_ = 0, end_ = 0, density_ = 0;
        uint64_t count_ = 0;
        double start() const { return start_; }
        double end() const { return end_; }
        uint64_t count() const { return count_; }
        double density() const { return density_; }
    };
    const std::vector<Bucket>& buckets() const { return buckets_; }
    size_t num_buckets() const { return buckets_.size(); }
    uint64_t num_samples() const { return samples_; }    // rows that landed in a bucket (NULL rows and NaN do not)
    bool has_density() const { return density_; }
    std::vector<Bucket> buckets_;
    uint64_t samples_ = 0;
    bool density_ = false;
};

// "Generic type that encapsulates vecs of primitive types" (src/table.rs:140-158): F / S / I
struct GenericVector {
    enum Kind { I, F, S } kind = I;
    std::vector<int64_t> i;
    std::vector<double> f;
    std::vector<std::string> s;
    size_t len() const { return kind == I ? i.size() : kind == F ? f.size() : s.size(); }
};

// ------------------------------------------------------------------------------------------------
// Column (src/table.rs:134-344)

struct Scalar;   // (Column::fill_null takes one; defined below)
struct ListArray;   // (Column::split returns one; defined with the ArrayFunctions)
class Column {
  public:
    Column() = default;
    Column(ChunkedArray data, Field field) : data_(std::move(data)), field_(std::move(field)) {}
    static Column from_arrays(std::vector<ArrayRef> arrays, Field field) {
        for (auto& a : arrays)
            if (a->dtype != field.data_type) throw DataFrameError(DataFrameError::ComputeError, "array type differs from the field's");
        return Column(ChunkedArray::from_arrays(std::move(arrays)), std::move(field));
    }
    const std::string& name() const { return field_.name; }
    DataType data_type() const { return field_.data_type; }
    const ChunkedArray& data() const { return data_; }
    const Field& field() const { return field_; }
    int64_t num_rows() const { return data_.num_rows(); }
    int64_t null_count() const { return data_.null_count(); }
    Column slice(int64_t offset, std::optional<int64_t> length = std::nullopt) const {
        if (data_type() == DataType::Utf8) {  // opaque host column: slice the strings
            std::vector<ArrayRef> out;
            int64_t len = std::min(length.value_or(INT64_MAX), num_rows());
            for (auto& c : data_.chunks()) {
                if (offset >= c->length) { offset -= c->length; continue; }
                if (len <= 0) break;
                const int64_t n = std::min(len, c->length - offset);
                out.push_back(Array::from_strings(std::vector<std::string>(c->strings->begin() + offset, c->strings->begin() + offset + n)));
                len -= n; offset = 0;
            }
            if (out.empty()) out.push_back(Array::from_strings({}));
            return Column(ChunkedArray::from_arrays(out), field_);
        }
        return Column(data_.slice(offset, length), field_);
    }
    Column filter(const Column& condition) const { return Column(data_.filter(condition.data()), field_); }  // :213-215
    // The conditional and NULL functions (rdf_coalesce .. rdf_null_test and, for Utf8 columns, rdf_utf8_coalesce /
    // rdf_utf8_case_when; defined below ScalarFunctions, which the numeric ones go through).  A literal is converted to the
    // column's type; a text column takes a Scalar::String.
    inline Column coalesce(const Column& other) const;          // this where it is not NULL, else other
    inline Column fill_null(const Scalar& value) const;         // coalesce(this, value)
    inline Column greatest(const Column& other) const;          // Spark's ordering: NaN above every number, NULLs skipped
    inline Column least(const Column& other) const;
    inline Column nanvl(const Column& other) const;             // Float32 / Float64: this unless it is NaN, then other
    inline Column is_in(const Column& set) const;                // Boolean, SQL's three-valued x IN (set): rdf_member_mask(IS_IN)
    inline Column is_null() const;                              // Boolean, never NULL; Utf8 columns by their rows' bitmap
    inline Column is_not_null() const;
    inline Column is_nan() const;
    // coalesce / CASE WHEN over text (rdf_utf8_coalesce / rdf_utf8_case_when), staged as concat stages its parts: a value is a
    // Utf8 column, a literal or the NULL literal; conds are Boolean columns of the same chunking (none: coalesce); `otherwise`
    // may be nullptr (NULL).  The result is an ordinary Utf8 column: a key for group_aggregate, joins and sort.
    struct TextValue {
        const Column* column = nullptr;
        std::string literal;
        bool null = false;
        TextValue(const Column& c) : column(&c) {}
        TextValue(std::string s) : literal(std::move(s)) {}
        TextValue(const char* s) : literal(s) {}
        static TextValue null_literal() { TextValue v(""); v.null = true; return v; }
    };
    static Column text_select(const std::vector<const Column*>& conds, const std::vector<TextValue>& values, const TextValue* otherwise, const std::string& name) {
        const bool cw = !conds.empty();
        const char* what = cw ? "when" : "coalesce";
        if (cw && conds.size() != values.size()) throw DataFrameError(DataFrameError::ComputeError, "when: one value per condition");
        std::vector<const TextValue*> slots;
        for (auto& v : values) slots.push_back(&v);
        if (otherwise) slots.push_back(otherwise);
        std::vector<TextChunks> tcs;
        tcs.reserve(slots.size());
        std::vector<rdf_utf8_part> cp;
        const Column* first = nullptr;
        for (auto* v : slots) {
            if (!v->column) { cp.push_back(rdf_utf8_part{nullptr, v->null ? nullptr : (const uint8_t*)v->literal.data(), v->null ? 0 : (int64_t)v->literal.size()}); continue; }
            v->column->need_text(what);
            if (!first) first = v->column;
            if (v->column->data_.num_chunks() != first->data_.num_chunks()) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": chunk lists differ in length");
            tcs.push_back(v->column->text_chunks(what));
            cp.push_back(rdf_utf8_part{tcs.back().txt.data(), nullptr, 0});
        }
        if (!first) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": at least one part must be a column");
        const size_t n = first->data_.num_chunks();
        // the conditions, on the host like the text: values and validity as bitmaps at offset 0
        std::vector<std::vector<uint8_t>> bits;
        std::vector<std::vector<rdf_array>> cviews(conds.size());
        bits.reserve(conds.size() * n * 2);
        for (size_t k = 0; k < conds.size(); ++k) {
            if (conds[k]->data_type() != DataType::Boolean) throw DataFrameError(DataFrameError::ComputeError, "when: a condition is a Boolean column");
            if (conds[k]->data_.num_chunks() != n) throw DataFrameError(DataFrameError::ComputeError, "when: chunk lists differ in length");
            for (auto& a : conds[k]->data_.chunks()) {
                bits.push_back(pack_bits(a->bools_to_host()));
                const uint8_t* vals = bits.back().data();
                const uint8_t* valid = nullptr;
                if (a->validity) { bits.push_back(pack_bits(a->valid_to_host())); valid = bits.back().data(); }
                cviews[k].push_back(rdf_array{vals, valid, 0, a->length, -1, RDF_BOOL, RDF_MEM_HOST});
            }
        }
        std::vector<const rdf_array*> cptr;
        for (auto& v : cviews) cptr.push_back(v.data());
        std::vector<bool> nullable(n, false);
        for (size_t i = 0; i < n; ++i) {
            bool any = cw && !otherwise, all = true;
            for (auto* v : slots) {
                const bool nl = v->column ? v->column->data_.chunk(i)->validity != nullptr : v->null;
                any = any || nl;
                all = all && nl;
            }
            nullable[i] = cw ? any : all;
        }
        const size_t nv = values.size();
        return text_build(tcs[0], nullable, name, [&](rdf_out* oo, rdf_out* od) {
            if (!cw) return rdf_utf8_coalesce(cp.data(), (int32_t)nv, (int64_t)n, oo, od);
            return rdf_utf8_case_when(cptr.data(), cp.data(), (int32_t)nv, otherwise ? &cp[nv] : nullptr, (int64_t)n, oo, od);
        });
    }
    Column renamed(const std::string& n) const { Column c = *this; c.field_.name = n; return c; }

    // src/table.rs:218-241: gather over the concatenation of the chunks; the result is ONE chunk whatever
    // chunk_size says.  indices: UInt32 (drop-in) or UInt64.
    Column take(const ArrayRef& indices, size_t chunk_size) const {
        if (data_type() == DataType::Utf8) {
            // text columns are carried on the host: gather there (a NULL index gives a NULL, i.e. an empty slot marked invalid)
            std::vector<const std::string*> flat;
            std::vector<bool> flat_valid;
            for (auto& c : data_.chunks()) {
                const std::vector<bool> v = c->valid_to_host();
                for (int64_t r = 0; r < c->length; ++r) { flat.push_back(&(*c->strings)[(size_t)(c->offset + r)]); flat_valid.push_back(v[(size_t)r]); }
            }
            const std::vector<bool> iv_valid = indices->valid_to_host();
            std::vector<uint64_t> idx;
            if (indices->dtype == DataType::UInt32) { for (uint32_t x : indices->values_to_host<uint32_t>()) idx.push_back(x); }
            else if (indices->dtype == DataType::UInt64) { for (uint64_t x : indices->values_to_host<uint64_t>()) idx.push_back(x); }
            else throw DataFrameError(DataFrameError::ComputeError, "take: indices must be UInt32 / UInt64");
            std::vector<std::string> out(idx.size());
            std::vector<bool> valid(idx.size(), true);
            bool any_null = false;
            for (size_t j = 0; j < idx.size(); ++j) {
                if (!iv_valid[j]) { valid[j] = false; any_null = true; continue; }
                if (idx[j] >= flat.size()) throw DataFrameError(DataFrameError::ComputeError, "take: index out of bounds");
                out[j] = *flat[(size_t)idx[j]];
                if (!flat_valid[(size_t)idx[j]]) { valid[j] = false; any_null = true; }
            }
            auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(out)));
            if (any_null) {
                const auto bits = pack_bits(valid);
                a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
                check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
                for (bool b : valid) a->null_count += !b;
            }
            return Column(ChunkedArray::from_arrays({ArrayRef(a)}), field_);
        }
        if (data_type() == DataType::Boolean) {   // Boolean columns travel through the gather as UInt8 (cast there and back on the device)
            const Column wide(ChunkedArray::from_arrays(cast_arrays(data_.chunks(), DataType::UInt8)), Field{field_.name, DataType::UInt8, field_.nullable});
            const Column taken = wide.take(indices, chunk_size);
            return Column(ChunkedArray::from_arrays(cast_arrays(taken.data().chunks(), DataType::Boolean)), field_);
        }
        const auto cv = data_.views();
        const rdf_array iv = indices->view();
        bool nullable = indices->validity != nullptr;
        for (auto& c : data_.chunks()) nullable |= c->validity != nullptr;
        bool host = indices->host;   // a host-resident column taken by host-resident indices (a grouped call's first rows): the result is host-resident too
        for (auto& c : data_.chunks()) host &= c->host;
        auto out = Array::make_out(data_type(), indices->length, nullable, host);
        rdf_out ov = out->out_view(indices->length);
        check(rdf_take(cv.data(), (int64_t)cv.size(), &iv, &ov));
        out->length = ov.length;
        out->null_count = ov.null_count;
        return Column(ChunkedArray::from_arrays({out}), field_);
    }
    // src/table.rs:244-290: Int64 / Float64 columns (the reference panics on the rest); NULL rows and NaN are not counted
    // (the reference reads the value slot of a NULL row: not copied).  The counting runs on the device (rdf_hist); the
    // density of a bucket is count / counted rows, computed here.
    Histogram hist(uint64_t nbins, bool density) const {
        if (data_type() != DataType::Int64 && data_type() != DataType::Float64)
            throw DataFrameError(DataFrameError::ComputeError, "Unsupported type for histogram");
        const auto cv = data_.views();
        bool host = true;
        for (auto& c : data_.chunks()) host &= c->host;
        auto counts = Array::make_out(DataType::Int64, (int64_t)nbins, false, host);
        auto edges = Array::make_out(DataType::Float64, (int64_t)nbins + 1, false, host);
        rdf_out oc = counts->out_view((int64_t)nbins), oe = edges->out_view((int64_t)nbins + 1);
        int64_t counted = 0;
        check(rdf_hist(cv.data(), (int64_t)cv.size(), (int64_t)nbins, nullptr, &oc, &oe, &counted));
        counts->length = oc.length;
        edges->length = oe.length;
        const std::vector<int64_t> c = counts->values_to_host<int64_t>();
        const std::vector<double> e = edges->values_to_host<double>();
        Histogram h;
        h.samples_ = (uint64_t)counted;
        h.density_ = density;
        h.buckets_.resize((size_t)nbins);
        for (size_t b = 0; b < (size_t)nbins; ++b) {
            h.buckets_[b].start_ = e[b];
            h.buckets_[b].end_ = e[b + 1];
            h.buckets_[b].count_ = (uint64_t)c[b];
            h.buckets_[b].density_ = density && counted > 0 ? (double)c[b] / (double)counted : 0.0;
        }
        return h;
    }

    // src/table.rs:293-341: the distinct values of the valid rows, in unspecified order (the reference's is HashSet order).
    // Int64 -> I, Float64 -> F (-0.0 and +0.0 one value, all NaNs one value), Utf8 -> S; other types panic in the reference.
    GenericVector uniques() const {
        GenericVector g;
        if (data_type() == DataType::Utf8) {
            const TextChunks tc = text_chunks("uniques");
            const std::vector<rdf_utf8_array>& txt = tc.txt;
            const int64_t rows = tc.rows, bytes = tc.bytes;
            // rows + 1 offsets and the input's bytes always suffice: one call
            std::vector<int32_t> ooffs((size_t)rows + 1, 0);
            std::vector<uint8_t> odata((size_t)bytes + 8, 0);
            rdf_out oo{ooffs.data(), nullptr, rows + 1, 0, 0, RDF_I32, RDF_MEM_HOST};
            rdf_out od{odata.data(), nullptr, bytes, 0, 0, RDF_U8, RDF_MEM_HOST};
            int64_t count = 0;
            check(rdf_utf8_uniques(txt.data(), (int64_t)txt.size(), &oo, &od, &count));
            g.kind = GenericVector::S;
            for (int64_t k = 0; k < count; ++k)
                g.s.emplace_back((const char*)odata.data() + ooffs[(size_t)k], (size_t)(ooffs[(size_t)k + 1] - ooffs[(size_t)k]));
            return g;
        }
        if (data_type() != DataType::Int64 && data_type() != DataType::Float64)
            throw DataFrameError(DataFrameError::ComputeError, "Datatype not supported for uniques.");
        const auto cv = data_.views();
        bool host = true;
        for (auto& c : data_.chunks()) host &= c->host;
        int64_t count = 0;
        check(rdf_uniques(cv.data(), (int64_t)cv.size(), nullptr, &count));
        auto out = Array::make_out(data_type(), count, false, host);
        rdf_out ov = out->out_view(count);
        check(rdf_uniques(cv.data(), (int64_t)cv.size(), &ov, &count));
        out->length = ov.length;
        if (data_type() == DataType::Int64) { g.kind = GenericVector::I; g.i = out->values_to_host<int64_t>(); }
        else { g.kind = GenericVector::F; g.f = out->values_to_host<double>(); }
        return g;
    }

    // {UInt32 codes with the input's chunking, Utf8 dictionary}: rdf_utf8_dictionary_encode.  A code is the rank of its value's
    // first occurrence over the whole column (pandas.factorize), a NULL row gives a NULL code, the dictionary holds every
    // distinct value once in that order; take() of the dictionary by a chunk of codes gives the chunk back.
    std::pair<Column, Column> dictionary_encode() const {
        if (data_type() != DataType::Utf8) throw DataFrameError(DataFrameError::ComputeError, "dictionary_encode: Utf8 columns only");
        const TextChunks tc = text_chunks("dictionary_encode");
        std::vector<std::shared_ptr<Array>> codes;
        std::vector<rdf_out> oc;
        for (auto& a : data_.chunks()) {
            codes.push_back(Array::make_out(DataType::UInt32, a->length, a->validity != nullptr, true));
            oc.push_back(codes.back()->out_view(a->length));
        }
        std::vector<int32_t> ooffs((size_t)tc.rows + 1, 0);
        std::vector<uint8_t> odata((size_t)tc.bytes + 8, 0);
        rdf_out oo{ooffs.data(), nullptr, tc.rows + 1, 0, 0, RDF_I32, RDF_MEM_HOST};
        rdf_out od{odata.data(), nullptr, tc.bytes, 0, 0, RDF_U8, RDF_MEM_HOST};
        int64_t count = 0;
        check(rdf_utf8_dictionary_encode(tc.txt.data(), (int64_t)tc.txt.size(), oc.data(), &oo, &od, &count));
        std::vector<ArrayRef> cc;
        for (size_t i = 0; i < codes.size(); ++i) { codes[i]->length = oc[i].length; codes[i]->null_count = oc[i].null_count; cc.push_back(codes[i]); }
        std::vector<std::string> dict;
        for (int64_t k = 0; k < count; ++k)
            dict.emplace_back((const char*)odata.data() + ooffs[(size_t)k], (size_t)(ooffs[(size_t)k + 1] - ooffs[(size_t)k]));
        return {Column::from_arrays(cc, Field{field_.name, DataType::UInt32, true}),
                Column::from_arrays({Array::from_strings(std::move(dict))}, Field{field_.name, DataType::Utf8, false})};
    }
  private:
    // text columns are carried on the host: every chunk as offsets + bytes built from the mirror's strings, in host memory
    struct TextChunks {
        struct Text { std::vector<int32_t> offs; std::string bytes; std::vector<uint8_t> valid; std::vector<std::shared_ptr<DeviceBuffer>> dev; };
        std::vector<std::unique_ptr<Text>> keep;
        std::vector<rdf_utf8_array> txt;
        int64_t rows = 0, bytes = 0;
    };
    // (host = false: the buffers are copied to the device, for calls whose other columns live there)
    TextChunks text_chunks(const char* what, bool host = true) const {
        using Text = TextChunks::Text;
        TextChunks tc;
        const int32_t mem = host ? RDF_MEM_HOST : RDF_MEM_DEVICE;
        auto place = [&](Text& t, const void* src, int64_t bytes) -> const void* {
            if (host) return src;
            t.dev.push_back(std::make_shared<DeviceBuffer>(bytes + 8));
            if (bytes > 0) check(rdf_copy_h2d(t.dev.back()->data(), src, bytes));
            return t.dev.back()->data();
        };
        for (auto& a : data_.chunks()) {
            tc.keep.push_back(std::make_unique<Text>());
            Text& t = *tc.keep.back();
            t.offs.reserve((size_t)a->length + 1);
            t.offs.push_back(0);
            for (int64_t r = 0; r < a->length; ++r) {
                t.bytes += (*a->strings)[(size_t)(a->offset + r)];
                if (t.bytes.size() > (size_t)INT32_MAX) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": a Utf8 chunk above 2^31-1 bytes");
                t.offs.push_back((int32_t)t.bytes.size());
            }
            if (a->validity) { t.valid = pack_bits(a->valid_to_host()); t.valid.resize(t.valid.size() + 8, 0); }
            t.bytes.append(8, '\0');
            rdf_utf8_array u;
            u.offsets.values = place(t, t.offs.data(), (int64_t)t.offs.size() * 4);
            u.offsets.validity = t.valid.empty() ? nullptr : (const uint8_t*)place(t, t.valid.data(), (int64_t)t.valid.size());
            u.offsets.offset = 0; u.offsets.length = a->length + 1; u.offsets.null_count = -1; u.offsets.dtype = RDF_I32; u.offsets.mem = mem;
            u.data.values = place(t, t.bytes.data(), (int64_t)t.bytes.size());
            u.data.validity = nullptr;
            u.data.offset = 0; u.data.length = (int64_t)t.bytes.size() - 8; u.data.null_count = 0; u.data.dtype = RDF_U8; u.data.mem = mem;
            tc.txt.push_back(u);
            tc.rows += a->length;
            tc.bytes += u.data.length;
        }
        return tc;
    }
    // One result array per text chunk, computed into host memory (text columns are host-carried, so the call is a host call)
    // and handed back in page-locked host memory (`on_host`) or on the device, where the frame's other columns are.
    template <class Call>
    Column text_result(DataType t, const TextChunks& tc, const std::vector<bool>& nullable, const std::string& name, bool on_host, Call call) const {
        const size_t n = tc.txt.size();
        std::vector<std::vector<uint8_t>> vals(n), valid(n);
        std::vector<rdf_out> ov(n);
        for (size_t i = 0; i < n; ++i) {
            const int64_t rows = tc.txt[i].offsets.length - 1, cap = (rows + 63) / 64 * 64;
            vals[i].assign((size_t)(t == DataType::Boolean ? cap / 8 + 8 : cap * type_size(t) + 8), 0);
            if (nullable[i]) valid[i].assign((size_t)(cap / 8 + 8), 0);
            ov[i] = rdf_out{vals[i].data(), nullable[i] ? valid[i].data() : nullptr, rows, 0, 0, (int32_t)t, RDF_MEM_HOST};
        }
        call(ov.data());
        std::vector<ArrayRef> res;
        for (size_t i = 0; i < n; ++i) {
            auto a = Array::make_out(t, ov[i].length, nullable[i], on_host);
            auto put = [&](const BufferRef& dst, const std::vector<uint8_t>& src) {
                if (on_host) std::memcpy(dst->data(), src.data(), src.size());
                else check(rdf_copy_h2d(dst->data(), src.data(), (int64_t)src.size()));
            };
            put(a->values, vals[i]);
            if (nullable[i]) put(a->validity, valid[i]);
            a->length = ov[i].length;
            a->null_count = ov[i].null_count;
            res.push_back(a);
        }
        return Column::from_arrays(res, Field{name, t, true});
    }
    void need_text(const char* what) const {
        if (data_type() != DataType::Utf8) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": Utf8 columns only");
    }
  public:
    // Masks and integers from text, on the device (rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure; SQL / Spark
    // semantics, see the C header).  A NULL row gives a NULL result.
    //   utf8_predicate  op = RDF_UTF8_EQ .. RDF_UTF8_LIKE against a literal / LIKE pattern (escape: -1 = none) -> Boolean
    //   utf8_compare    op = RDF_UTF8_EQ .. RDF_UTF8_GE against another Utf8 column with the same chunking      -> Boolean
    //   utf8_measure    RDF_UTF8_LENGTH / OCTET_LENGTH / LOCATE (needle, 1-based code-point position `pos`)      -> Int32
    Column utf8_predicate(int32_t op, const std::string& pattern, int32_t escape = -1, bool on_host = false) const {
        need_text("utf8_predicate");
        const TextChunks tc = text_chunks("utf8_predicate");
        std::vector<bool> nullable;
        for (auto& a : data_.chunks()) nullable.push_back(a->validity != nullptr);
        return text_result(DataType::Boolean, tc, nullable, "bool_filter", on_host, [&](rdf_out* outs) {
            check(rdf_utf8_predicate(op, tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)pattern.data(), (int64_t)pattern.size(), escape, outs));
        });
    }
    Column utf8_compare(int32_t op, const Column& other, bool on_host = false) const {
        need_text("utf8_compare");
        other.need_text("utf8_compare");
        if (other.data_.num_chunks() != data_.num_chunks()) throw DataFrameError(DataFrameError::ComputeError, "utf8_compare: chunk lists differ in length");
        const TextChunks ta = text_chunks("utf8_compare"), tb = other.text_chunks("utf8_compare");
        std::vector<bool> nullable;
        for (size_t i = 0; i < data_.num_chunks(); ++i) nullable.push_back(data_.chunk(i)->validity != nullptr || other.data_.chunk(i)->validity != nullptr);
        return text_result(DataType::Boolean, ta, nullable, "bool_filter", on_host, [&](rdf_out* outs) {
            check(rdf_utf8_compare(op, ta.txt.data(), tb.txt.data(), (int64_t)ta.txt.size(), outs));
        });
    }
    Column utf8_measure(int32_t what, const std::string& pattern = std::string(), int64_t pos = 1, bool on_host = false) const {
        need_text("utf8_measure");
        const TextChunks tc = text_chunks("utf8_measure");
        std::vector<bool> nullable;
        for (auto& a : data_.chunks()) nullable.push_back(a->validity != nullptr);
        return text_result(DataType::Int32, tc, nullable, field_.name, on_host, [&](rdf_out* outs) {
            check(rdf_utf8_measure(what, tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)pattern.data(), (int64_t)pattern.size(), pos, outs));
        });
    }

    // Text to values and back, on the device (rdf_utf8_parse / rdf_utf8_format; Spark 3's semantics as the C header states them).
    //   utf8_parse    this Utf8 column -> Boolean / an integer type / Int32 day numbers / Int64 timestamps in `unit`; pattern null:
    //                 the kind's CAST grammar, else to_date / to_timestamp / unix_timestamp.  A row that does not parse is NULL,
    //                 so every result chunk carries a bitmap.
    //   utf8_format   Boolean / integer / temporal storage chunks -> a Utf8 column carried like every text column of this mirror
    //                 (the values are staged through the host, as text is); pattern null: CAST(x AS STRING), else date_format.
    Column utf8_parse(rdf_text_kind kind, DataType out, int32_t unit = RDF_TIME_SECOND, const std::string* pattern = nullptr, bool on_host = false) const {
        need_text("utf8_parse");
        const TextChunks tc = text_chunks("utf8_parse");
        const std::vector<bool> nullable(tc.txt.size(), true);
        return text_result(out, tc, nullable, field_.name, on_host, [&](rdf_out* outs) {
            check(rdf_utf8_parse(tc.txt.data(), (int64_t)tc.txt.size(), (int32_t)kind, unit, pattern ? (const uint8_t*)pattern->data() : nullptr,
                                 pattern ? (int64_t)pattern->size() : 0, outs, nullptr));
        });
    }
    static Column utf8_format(const std::vector<ArrayRef>& arr, rdf_text_kind kind, int32_t unit = RDF_TIME_SECOND, const std::string* pattern = nullptr,
                              const std::string& name = "format") {
        return format_staged(arr, name, "utf8_format", [&](const rdf_array* a, int64_t n, rdf_out* oo, rdf_out* od) {
            return rdf_utf8_format(a, n, (int32_t)kind, unit, pattern ? (const uint8_t*)pattern->data() : nullptr, pattern ? (int64_t)pattern->size() : 0, oo, od);
        });
    }
    // Float32 / Float64 to and from text, on the device (rdf_utf8_parse_float / rdf_utf8_format_float): correctly rounded
    // parsing, a row that does not parse is NULL; Java's Double.toString / Float.toString.
    Column utf8_parse_float(DataType out, bool on_host = false) const {
        need_text("utf8_parse_float");
        const TextChunks tc = text_chunks("utf8_parse_float");
        const std::vector<bool> nullable(tc.txt.size(), true);
        return text_result(out, tc, nullable, field_.name, on_host, [&](rdf_out* outs) {
            check(rdf_utf8_parse_float(tc.txt.data(), (int64_t)tc.txt.size(), outs, nullptr));
        });
    }
    Column utf8_format_float() const { return utf8_format_float(data_.chunks(), field_.name); }
    static Column utf8_format_float(const std::vector<ArrayRef>& arr, const std::string& name = "format") {
        return format_staged(arr, name, "utf8_format_float", [&](const rdf_array* a, int64_t n, rdf_out* oo, rdf_out* od) { return rdf_utf8_format_float(a, n, oo, od); });
    }
  private:
    // value chunks staged through the host (as text is), then `call` under the sizing rule -> a Utf8 column
    template <class F>
    static Column format_staged(const std::vector<ArrayRef>& arr, const std::string& name, const char* what, F call) {
        struct Staged { std::vector<uint8_t> values, valid; };
        std::vector<Staged> keep(arr.size());
        std::vector<rdf_array> a;
        std::vector<bool> nullable;
        TextChunks shape;
        for (size_t i = 0; i < arr.size(); ++i) {
            const Array& x = *arr[i];
            if (x.dtype == DataType::Utf8) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": the input is text already");
            Staged& s = keep[i];
            if (x.dtype == DataType::Boolean) s.values = pack_bits(x.bools_to_host());
            else {
                const int64_t es = (int64_t)type_size(x.dtype);
                s.values.resize((size_t)(x.length * es));
                if (x.length > 0) x.fetch(s.values.data(), (const uint8_t*)x.values->data() + x.offset * es, x.length * es);
            }
            s.values.resize(s.values.size() + 8, 0);
            if (x.validity) { s.valid = pack_bits(x.valid_to_host()); s.valid.resize(s.valid.size() + 8, 0); }
            a.push_back(rdf_array{s.values.data(), x.validity ? s.valid.data() : nullptr, 0, x.length, x.validity ? x.null_count : 0, (int32_t)x.dtype, RDF_MEM_HOST});
            rdf_utf8_array u;
            std::memset(&u, 0, sizeof u);
            u.offsets.length = x.length + 1;
            shape.txt.push_back(u);
            nullable.push_back(x.validity != nullptr);
        }
        return text_build(shape, nullable, name, [&](rdf_out* oo, rdf_out* od) { return call(a.data(), (int64_t)a.size(), oo, od); });
    }
  public:
    // to_date(s, fmt) / to_timestamp(s, fmt) / unix_timestamp(s, fmt) of a Utf8 column; date_format / from_unix_time of a temporal one
    Column to_date(const std::string& fmt) const { return utf8_parse(RDF_TEXT_DATE, DataType::Int32, RDF_TIME_SECOND, &fmt); }
    Column to_timestamp(rdf_time_unit unit, const std::string& fmt) const { return utf8_parse(RDF_TEXT_TIMESTAMP, DataType::Int64, (int32_t)unit, &fmt); }
    Column unix_timestamp(const std::string& fmt) const { return utf8_parse(RDF_TEXT_TIMESTAMP, DataType::Int64, RDF_TIME_SECOND, &fmt); }
    Column date_format(rdf_time_unit unit, const std::string& fmt) const { return utf8_format(data_.chunks(), RDF_TEXT_TIMESTAMP, (int32_t)unit, &fmt, field_.name); }
    Column from_unix_time(const std::string& fmt) const { return utf8_format(data_.chunks(), RDF_TEXT_TIMESTAMP, RDF_TIME_SECOND, &fmt, field_.name); }
    // CAST between Utf8 and Boolean / the integer types / Float32 / Float64 (either direction)
    Column cast_text(DataType to) const {
        if (data_type() == DataType::Utf8) {
            if (is_float(to)) return utf8_parse_float(to);
            if (to != DataType::Boolean && !is_integer_type(to)) throw DataFrameError(DataFrameError::ComputeError, "cast: Utf8 casts to Boolean, the integer types and the float types");
            return utf8_parse(to == DataType::Boolean ? RDF_TEXT_BOOL : RDF_TEXT_INT, to);
        }
        if (to == DataType::Utf8 && is_float(data_type())) return utf8_format_float(data_.chunks(), field_.name);
        if (to != DataType::Utf8 || (data_type() != DataType::Boolean && !is_integer_type(data_type())))
            throw DataFrameError(DataFrameError::ComputeError, "cast: Boolean, the integer types and the float types cast to Utf8");
        return utf8_format(data_.chunks(), data_type() == DataType::Boolean ? RDF_TEXT_BOOL : RDF_TEXT_INT, RDF_TIME_SECOND, nullptr, field_.name);
    }
    static bool is_integer_type(DataType t) { return (int32_t)t >= RDF_I8 && (int32_t)t <= RDF_U64; }

    // Text columns made of more than one source, on the device (rdf_utf8_concat / _pad / _repeat / _reverse /
    // _substring_index; Spark 3's semantics, see the C header): each call runs twice under the sizing rule and returns an
    // ordinary Utf8 column with the input's chunking, carried like every text column of this mirror, so with_column,
    // group_aggregate, joins and sort take it as a key as it is.
    //   concat / concat_ws   parts are Utf8 columns of one chunking and literals; concat is NULL where a column part is,
    //                        concat_ws skips NULL parts and is never NULL
    //   lpad / rpad          to `len` code points with the pad cycled; a longer row is truncated
    //   repeat, reverse, substring_index(delim, count)   (count < 0 counts from the right; occurrences may overlap)
    struct Utf8Part {
        const Column* column = nullptr;
        std::string literal;
        Utf8Part(const Column& c) : column(&c) {}
        Utf8Part(std::string s) : literal(std::move(s)) {}
        Utf8Part(const char* s) : literal(s) {}
    };
    static Column concat(const std::vector<Utf8Part>& parts, const std::string& name = "concat") { return concat_parts(parts, false, std::string(), name); }
    static Column concat_ws(const std::string& sep, const std::vector<Utf8Part>& parts, const std::string& name = "concat_ws") { return concat_parts(parts, true, sep, name); }
    Column lpad(int64_t len, const std::string& pad) const { return pad_side(0, len, pad); }
    Column rpad(int64_t len, const std::string& pad) const { return pad_side(1, len, pad); }
    Column repeat(int64_t times) const {
        need_text("repeat");
        const TextChunks tc = text_chunks("repeat");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) { return rdf_utf8_repeat(tc.txt.data(), (int64_t)tc.txt.size(), times, oo, od); });
    }
    Column reverse() const {
        need_text("reverse");
        const TextChunks tc = text_chunks("reverse");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) { return rdf_utf8_reverse(tc.txt.data(), (int64_t)tc.txt.size(), oo, od); });
    }
    Column substring_index(const std::string& delim, int64_t count) const {
        need_text("substring_index");
        const TextChunks tc = text_chunks("substring_index");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_substring_index(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)delim.data(), (int64_t)delim.size(), count, oo, od);
        });
    }

    // A row's content changed by what the row holds, on the device (rdf_utf8_replace / _translate / _initcap / _split; Spark 3's
    // semantics, see the C header): each call runs twice under the sizing rule.  replace, translate and initcap return an
    // ordinary Utf8 column with the input's chunking, a key for group_aggregate, joins and sort like any other.
    //   replace(search, replacement)   every non-overlapping occurrence from the left; an empty search changes nothing
    //   translate(matching, replace)   code point i of matching becomes code point i of replace, or is dropped
    //   initcap()                      lower-cased; the first code point of the row and after every ' ' title-cased
    //   split(delim, limit)            a LITERAL delimiter -> ONE ListArray over all chunks with a Utf8 child (text stays on the
    //                                  host in this mirror), which ScalarFunctions::explode takes; defined below ListArray
    Column replace(const std::string& search, const std::string& replacement) const {
        need_text("replace");
        const TextChunks tc = text_chunks("replace");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_replace(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)search.data(), (int64_t)search.size(),
                                    (const uint8_t*)replacement.data(), (int64_t)replacement.size(), oo, od);
        });
    }
    Column translate(const std::string& matching, const std::string& replace) const {
        need_text("translate");
        const TextChunks tc = text_chunks("translate");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_translate(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)matching.data(), (int64_t)matching.size(),
                                      (const uint8_t*)replace.data(), (int64_t)replace.size(), oo, od);
        });
    }
    Column initcap() const {
        need_text("initcap");
        const TextChunks tc = text_chunks("initcap");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) { return rdf_utf8_initcap(tc.txt.data(), (int64_t)tc.txt.size(), oo, od); });
    }
    inline ListArray split(const std::string& delim, int64_t limit = -1) const;
    // The median and the p-quantile (Spark's `percentile`: linear between the two nearest ranks) of a numeric column over its
    // non-NULL rows, none for a column without one: AggregateFunctions::median / percentile (rdf_groupby_percentile).
    inline std::optional<double> median() const;
    inline std::optional<double> quantile(double p) const;

    // Regular expressions, on the device (rdf_utf8_regexp_match / _count / _extract / _replace / _split; java.util.regex's
    // leftmost-first matching over the accepted syntax, see the C header): a pattern outside it, or past a size cap, throws
    // before any device work.  A NULL row gives NULL.
    //   rlike(pattern)                  a match exists anywhere in the row                                      -> Boolean
    //   regexp_count(pattern)           the matches Matcher.find finds                                          -> Int32
    //   regexp_extract(pattern, 0)      the first match, or "" (group != 0 throws: capture groups are not built) -> Utf8
    //   regexp_replace(pattern, rep)    every match replaced; `\x` in rep stands for x, an unescaped `$` throws -> Utf8
    //   split_regexp(pattern, limit)    String.split(regex, limit) -> ONE ListArray as split() returns it; defined below ListArray
    Column rlike(const std::string& pattern, bool on_host = false) const {
        need_text("rlike");
        const TextChunks tc = text_chunks("rlike");
        return text_result(DataType::Boolean, tc, chunk_nullable(), "bool_filter", on_host, [&](rdf_out* outs) {
            check(rdf_utf8_regexp_match(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)pattern.data(), (int64_t)pattern.size(), outs));
        });
    }
    Column regexp_count(const std::string& pattern, bool on_host = false) const {
        need_text("regexp_count");
        const TextChunks tc = text_chunks("regexp_count");
        return text_result(DataType::Int32, tc, chunk_nullable(), field_.name, on_host, [&](rdf_out* outs) {
            check(rdf_utf8_regexp_count(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)pattern.data(), (int64_t)pattern.size(), outs));
        });
    }
    Column regexp_extract(const std::string& pattern, int32_t group = 0) const {
        need_text("regexp_extract");
        const TextChunks tc = text_chunks("regexp_extract");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_regexp_extract(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)pattern.data(), (int64_t)pattern.size(), group, oo, od);
        });
    }
    Column regexp_replace(const std::string& pattern, const std::string& replacement) const {
        need_text("regexp_replace");
        const TextChunks tc = text_chunks("regexp_replace");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_regexp_replace(tc.txt.data(), (int64_t)tc.txt.size(), (const uint8_t*)pattern.data(), (int64_t)pattern.size(),
                                           (const uint8_t*)replacement.data(), (int64_t)replacement.size(), oo, od);
        });
    }
    inline ListArray split_regexp(const std::string& pattern, int64_t limit = -1) const;
    // split() and split_regexp(): `call(chunks, nchunks, list offsets, element offsets, data)` run twice under the sizing rule
    template <class Call> inline ListArray split_lists(const char* what, Call call) const;

    // Row hashes and digests, on the device (rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32; Spark 3's semantics, see the
    // C header).
    //   hash / xxhash64   Spark's Murmur3_x86_32 / XXH64 over the columns in order with a seed (42 is Spark's), NULLs skipped:
    //                     an ordinary Int32 / Int64 column that is never NULL, a key for group_aggregate, joins, windows
    //   md5 / sha1 / sha2(bits) / crc32   of a Utf8 column: lowercase hex text / Int64; a NULL row gives NULL.  sha2 takes
    //                     bits 0 (= 256), 224, 256, 384, 512 and refuses anything else (Spark returns NULL there)
    static Column hash_columns(int32_t kind, const std::vector<const Column*>& cols, int64_t seed = 42, const std::string& name = "hash") {
        if (cols.empty()) throw DataFrameError(DataFrameError::ComputeError, "hash: at least one column");
        const DataType t = kind == RDF_HASH_XXHASH64 ? DataType::Int64 : DataType::Int32;
        const size_t nch = cols[0]->data_.num_chunks();
        // the call runs where the numeric columns are (text is host-carried and copied there); text alone: on the device,
        // where a frame's numeric columns usually live, so that the result is a key next to them
        bool host = true, any_numeric = false;
        for (const Column* c : cols) {
            if (c->data_.num_chunks() != nch) throw DataFrameError(DataFrameError::ComputeError, "hash: chunk lists differ in length");
            if (c->data_type() != DataType::Utf8)
                for (auto& a : c->data_.chunks()) { host &= a->host; any_numeric = true; }
        }
        if (!any_numeric) host = false;
        std::vector<TextChunks> tcs;
        tcs.reserve(cols.size());
        std::vector<std::vector<rdf_array>> num(cols.size());
        std::vector<rdf_sort_key> keys(cols.size());
        for (size_t k = 0; k < cols.size(); ++k) {
            keys[k] = rdf_sort_key{nullptr, nullptr, rdf_sort_options{0, 0}};
            if (cols[k]->data_type() == DataType::Utf8) {
                tcs.push_back(cols[k]->text_chunks("hash", host));
                keys[k].utf8 = tcs.back().txt.data();
            } else {
                for (auto& a : cols[k]->data_.chunks()) num[k].push_back(a->view());
                keys[k].values = num[k].data();
            }
        }
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& a : cols[0]->data_.chunks()) {
            outs.push_back(Array::make_out(t, a->length, false, host));
            ov.push_back(outs.back()->out_view(a->length));
        }
        if (nch > 0) check(rdf_hash_columns(kind, keys.data(), (int32_t)keys.size(), (int64_t)nch, seed, ov.data()));
        std::vector<ArrayRef> res;
        for (size_t i = 0; i < outs.size(); ++i) { outs[i]->length = ov[i].length; outs[i]->null_count = 0; res.push_back(outs[i]); }
        return Column::from_arrays(res, Field{name, t, false});
    }
    Column hash(int64_t seed = 42) const { return hash_columns(RDF_HASH_MURMUR3_32, {this}, seed, field_.name); }
    Column xxhash64(int64_t seed = 42) const { return hash_columns(RDF_HASH_XXHASH64, {this}, seed, field_.name); }
    Column utf8_digest(int32_t kind, const char* what) const {
        need_text(what);
        const TextChunks tc = text_chunks(what);
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) { return rdf_utf8_digest(kind, tc.txt.data(), (int64_t)tc.txt.size(), oo, od); });
    }
    Column md5() const { return utf8_digest(RDF_DIGEST_MD5, "md5"); }
    Column sha1() const { return utf8_digest(RDF_DIGEST_SHA1, "sha1"); }
    Column sha2(int32_t bits) const {
        switch (bits) {
            case 0: case 256: return utf8_digest(RDF_DIGEST_SHA256, "sha2");
            case 224: return utf8_digest(RDF_DIGEST_SHA224, "sha2");
            case 384: return utf8_digest(RDF_DIGEST_SHA384, "sha2");
            case 512: return utf8_digest(RDF_DIGEST_SHA512, "sha2");
            default: throw DataFrameError(DataFrameError::ComputeError, "sha2: bits must be 0, 224, 256, 384 or 512");
        }
    }
    Column crc32(bool on_host = false) const {
        need_text("crc32");
        const TextChunks tc = text_chunks("crc32");
        return text_result(DataType::Int64, tc, chunk_nullable(), field_.name, on_host, [&](rdf_out* outs) {
            check(rdf_utf8_crc32(tc.txt.data(), (int64_t)tc.txt.size(), outs));
        });
    }
  private:
    inline Column text_null_test(int32_t op) const;
    std::vector<bool> chunk_nullable() const {
        std::vector<bool> nullable;
        for (auto& a : data_.chunks()) nullable.push_back(a->validity != nullptr);
        return nullable;
    }
    Column pad_side(int32_t side, int64_t len, const std::string& pad) const {
        need_text(side ? "rpad" : "lpad");
        const TextChunks tc = text_chunks(side ? "rpad" : "lpad");
        return text_build(tc, chunk_nullable(), field_.name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_pad(side, tc.txt.data(), (int64_t)tc.txt.size(), len, (const uint8_t*)pad.data(), (int64_t)pad.size(), oo, od);
        });
    }
    static Column concat_parts(const std::vector<Utf8Part>& parts, bool ws, const std::string& sep, const std::string& name) {
        const char* what = ws ? "concat_ws" : "concat";
        std::vector<TextChunks> tcs;
        tcs.reserve(parts.size());
        std::vector<rdf_utf8_part> cp;
        const Column* first = nullptr;
        for (auto& p : parts) {
            if (!p.column) { cp.push_back(rdf_utf8_part{nullptr, (const uint8_t*)p.literal.data(), (int64_t)p.literal.size()}); continue; }
            p.column->need_text(what);
            if (!first) first = p.column;
            if (p.column->data_.num_chunks() != first->data_.num_chunks()) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": chunk lists differ in length");
            tcs.push_back(p.column->text_chunks(what));
            cp.push_back(rdf_utf8_part{tcs.back().txt.data(), nullptr, 0});
        }
        if (!first) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": at least one part must be a column");
        std::vector<bool> nullable(first->data_.num_chunks(), false);
        if (!ws)
            for (auto& p : parts)
                if (p.column)
                    for (size_t i = 0; i < nullable.size(); ++i) nullable[i] = nullable[i] || p.column->data_.chunk(i)->validity != nullptr;
        return text_build(tcs[0], nullable, name, [&](rdf_out* oo, rdf_out* od) {
            return rdf_utf8_concat(cp.data(), (int32_t)cp.size(), (int64_t)nullable.size(), ws ? 1 : 0, (const uint8_t*)sep.data(), (int64_t)sep.size(), oo, od);
        });
    }
    // One Utf8 result chunk per text chunk of `shape`: the sizing call, then the call into exactly sized host buffers
    template <class Call>
    static Column text_build(const TextChunks& shape, const std::vector<bool>& nullable, const std::string& name, Call call) {
        const size_t n = shape.txt.size();
        std::vector<std::vector<int32_t>> offs(n);
        std::vector<std::vector<uint8_t>> valid(n), data(n);
        std::vector<rdf_out> oo(n), od(n);
        for (size_t i = 0; i < n; ++i) {
            const int64_t rows = shape.txt[i].offsets.length - 1;
            offs[i].assign((size_t)rows + 1, 0);
            if (nullable[i]) valid[i].assign((size_t)((rows + 63) / 64 * 8 + 8), 0);
            oo[i] = rdf_out{offs[i].data(), nullable[i] ? valid[i].data() : nullptr, rows + 1, 0, 0, RDF_I32, RDF_MEM_HOST};
            od[i] = rdf_out{nullptr, nullptr, 0, 0, 0, RDF_U8, RDF_MEM_HOST};
        }
        rdf_status st = call(oo.data(), od.data());
        if (st == RDF_MEMORY_ERROR) {
            for (size_t i = 0; i < n; ++i) {
                data[i].assign((size_t)od[i].length + 8, 0);
                od[i].values = data[i].data();
                od[i].capacity = od[i].length;
            }
            st = call(oo.data(), od.data());
        }
        check(st);
        std::vector<ArrayRef> res;
        bool any_null = false;
        for (size_t i = 0; i < n; ++i) {
            const int64_t rows = oo[i].length - 1;
            std::vector<std::string> strs((size_t)rows);
            for (int64_t r = 0; r < rows; ++r)
                strs[(size_t)r].assign((const char*)data[i].data() + offs[i][(size_t)r], (size_t)(offs[i][(size_t)r + 1] - offs[i][(size_t)r]));
            auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(strs)));
            if (nullable[i]) {
                const size_t nb = (size_t)((rows + 63) / 64 * 8);
                a->validity = std::make_shared<DeviceBuffer>((int64_t)nb + 8);
                check(rdf_copy_h2d(a->validity->data(), valid[i].data(), (int64_t)nb + 8));
                a->null_count = oo[i].null_count;
                any_null = true;
            }
            res.push_back(a);
        }
        if (res.empty()) res.push_back(Array::from_strings({}));
        return Column::from_arrays(res, Field{name, DataType::Utf8, any_null});
    }
    ChunkedArray data_;
    Field field_;
};

// ------------------------------------------------------------------------------------------------
// Scalar / BooleanFilter (src/expression.rs:718-870)

struct Scalar {
    enum Kind { Null, Int32, Int64, Float32, Float64, Boolean, String } kind = Null;   // Scalar::String: src/expression.rs:725,797-802
    double f = 0;
    int64_t i = 0;
    std::string s;
    Scalar() = default;
    Scalar(std::string v) : kind(String), s(std::move(v)) {}
    Scalar(const char* v) : kind(String), s(v) {}   // (without it a string literal picks the bool constructor)
    Scalar(int32_t v) : kind(Int32), i(v) {}
    Scalar(int64_t v) : kind(Int64), i(v) {}
    Scalar(float v) : kind(Float32), f(v) {}
    Scalar(double v) : kind(Float64), f(v) {}
    Scalar(bool v) : kind(Boolean), i(v) {}
    int32_t rdf_type() const {
        switch (kind) { case Int32: return RDF_I32; case Int64: return RDF_I64; case Float32: return RDF_F32;
                        case Float64: return RDF_F64; case Boolean: return RDF_BOOL; default: return RDF_NULLTYPE; }
    }
};

struct BooleanFilter;
using FilterRef = std::shared_ptr<const BooleanFilter>;
struct BooleanFilter {
    enum Kind { InputScalar, InputColumn, Not, And, Or, Gt, Ge, Eq, Ne, Lt, Le, StartsWith, EndsWith, Contains, Like, RLike, IsIn } kind;
    Scalar scalar_v;
    std::string column_name;
    std::shared_ptr<const Column> set_v;   // IsIn: the values (a column of the tested column's type)
    int32_t escape = -1;   // Like: -1 = none, or one ASCII byte
    FilterRef l, r;
    static FilterRef scalar(Scalar s) { auto f = std::make_shared<BooleanFilter>(); f->kind = InputScalar; f->scalar_v = s; return f; }
    static FilterRef column(const std::string& name) { auto f = std::make_shared<BooleanFilter>(); f->kind = InputColumn; f->column_name = name; return f; }
    static FilterRef make(Kind k, FilterRef a, FilterRef b = nullptr) { auto f = std::make_shared<BooleanFilter>(); f->kind = k; f->l = std::move(a); f->r = std::move(b); return f; }
    static FilterRef gt(FilterRef a, FilterRef b) { return make(Gt, a, b); }
    static FilterRef ge(FilterRef a, FilterRef b) { return make(Ge, a, b); }
    static FilterRef eq(FilterRef a, FilterRef b) { return make(Eq, a, b); }
    static FilterRef ne(FilterRef a, FilterRef b) { return make(Ne, a, b); }
    static FilterRef lt(FilterRef a, FilterRef b) { return make(Lt, a, b); }
    static FilterRef le(FilterRef a, FilterRef b) { return make(Le, a, b); }
    static FilterRef and_(FilterRef a, FilterRef b) { return make(And, a, b); }
    static FilterRef or_(FilterRef a, FilterRef b) { return make(Or, a, b); }
    static FilterRef not_(FilterRef a) { return make(Not, a); }
    // text predicates: a Utf8 column against a String scalar (SQL LIKE: '%' any run, '_' one code point, `escape` or -1)
    static FilterRef starts_with(FilterRef a, FilterRef b) { return make(StartsWith, a, b); }
    static FilterRef ends_with(FilterRef a, FilterRef b) { return make(EndsWith, a, b); }
    static FilterRef contains(FilterRef a, FilterRef b) { return make(Contains, a, b); }
    static FilterRef like(FilterRef a, FilterRef b, int32_t escape = -1) {
        auto f = std::make_shared<BooleanFilter>(); f->kind = Like; f->l = std::move(a); f->r = std::move(b); f->escape = escape; return f;
    }
    // RLIKE: the String scalar is a regular expression (rdf_utf8_regexp_match), true where a match exists anywhere in the row
    static FilterRef rlike(FilterRef a, FilterRef b) { return make(RLike, a, b); }
    // SQL's three-valued `column IN (set)` (rdf_member_mask, IS_IN): a NULL result drops the row like FALSE; NOT IN is not_(is_in(..))
    static FilterRef is_in(FilterRef column, const Column& set) {
        auto f = std::make_shared<BooleanFilter>(); f->kind = IsIn; f->l = std::move(column); f->set_v = std::make_shared<const Column>(set); return f;
    }
};

// ------------------------------------------------------------------------------------------------
// expression trees over named columns, lowered to rdf_expr_node arrays

struct Expr;
using ExprRef = std::shared_ptr<const Expr>;
struct Expr {
    enum Kind { Col, Lit, Op } kind = Col;
    std::string column;  // Col
    Scalar lit;          // Lit
    int32_t lit_type = RDF_F64;
    int32_t op = 0;      // Op (rdf_op)
    int32_t cast_to = 0;
    ExprRef l, r;
    static ExprRef col(const std::string& n) { auto e = std::make_shared<Expr>(); e->kind = Col; e->column = n; return e; }
    static ExprRef literal(Scalar s, int32_t as_type) { auto e = std::make_shared<Expr>(); e->kind = Lit; e->lit = s; e->lit_type = as_type; return e; }
    static ExprRef make(int32_t op, ExprRef a, ExprRef b = nullptr, int32_t cast_to = 0) {
        auto e = std::make_shared<Expr>(); e->kind = Op; e->op = op; e->l = std::move(a); e->r = std::move(b); e->cast_to = cast_to; return e;
    }
    bool has_divide() const { return kind == Op && (op == RDF_OP_DIV || (l && l->has_divide()) || (r && r->has_divide())); }
};

inline ExprRef filter_to_expr(const FilterRef& f, const std::function<ExprRef(const std::string&)>& resolve) {
    switch (f->kind) {
        case BooleanFilter::InputScalar:
            if (f->scalar_v.kind == Scalar::String) throw DataFrameError(DataFrameError::ComputeError, "a String scalar compares with Utf8 columns only");
            return Expr::literal(f->scalar_v, f->scalar_v.rdf_type());
        case BooleanFilter::StartsWith: case BooleanFilter::EndsWith: case BooleanFilter::Contains: case BooleanFilter::Like: case BooleanFilter::RLike:
            throw DataFrameError(DataFrameError::ComputeError, "starts_with / ends_with / contains / like / rlike take a Utf8 column and a String scalar");
        case BooleanFilter::InputColumn: return resolve(f->column_name);
        case BooleanFilter::Not: return Expr::make(RDF_OP_NOT, filter_to_expr(f->l, resolve));
        default: break;
    }
    static const std::map<int, int> ops = {{BooleanFilter::And, RDF_OP_AND}, {BooleanFilter::Or, RDF_OP_OR}, {BooleanFilter::Gt, RDF_OP_GT},
                                            {BooleanFilter::Ge, RDF_OP_GE}, {BooleanFilter::Eq, RDF_OP_EQ}, {BooleanFilter::Ne, RDF_OP_NE},
                                            {BooleanFilter::Lt, RDF_OP_LT}, {BooleanFilter::Le, RDF_OP_LE}};
    return Expr::make(ops.at(f->kind), filter_to_expr(f->l, resolve), filter_to_expr(f->r, resolve));
}

// Lowered program: node array + the distinct columns it reads (in first-use order).
struct Lowered {
    std::vector<rdf_expr_node> nodes;
    std::vector<std::string> columns;
    int add(const ExprRef& e) {
        rdf_expr_node n;
        std::memset(&n, 0, sizeof n);
        n.lhs = n.rhs = -1;
        if (e->kind == Expr::Col) {
            int idx = -1;
            for (size_t i = 0; i < columns.size(); ++i) if (columns[i] == e->column) idx = (int)i;
            if (idx < 0) { idx = (int)columns.size(); columns.push_back(e->column); }
            n.kind = RDF_NODE_COLUMN; n.column = idx;
        } else if (e->kind == Expr::Lit) {
            n.kind = RDF_NODE_SCALAR; n.dtype = e->lit.kind == Scalar::Null ? RDF_NULLTYPE : e->lit_type;
            const bool lit_is_float = e->lit.kind == Scalar::Float32 || e->lit.kind == Scalar::Float64;
            n.f64 = lit_is_float ? e->lit.f : (double)e->lit.i;
            n.i64 = lit_is_float ? (int64_t)e->lit.f : e->lit.i;
        } else {
            const int l = add(e->l);
            const int r = e->r ? add(e->r) : -1;
            n.kind = RDF_NODE_OP; n.op = e->op; n.lhs = l; n.rhs = r; n.dtype = e->cast_to;
        }
        nodes.push_back(n);
        return (int)nodes.size() - 1;
    }
};

// ------------------------------------------------------------------------------------------------
// plan types (src/expression.rs:286-712) and operation builders (src/operation/scalar.rs)

// ------------------------------------------------------------------------------------------------
// CSV text -> typed column buffers, on the host (DataFrame::from_csv, plan::Reader::get_dataset): arrow::csv::Reader with an
// inferred schema (src/dataframe.rs:349-389).  The file is read ONCE into memory and indexed by record; the types are
// inferred and the cells parsed by worker threads over ranges of records (std::from_chars: exact, locale-free), numbers land
// straight in the caller's (page-locked) column buffers.  A column whose non-empty cells all parse as integers is Int64, as
// numbers Float64, as true / false Boolean, anything else Utf8; an empty cell is a NULL.  Quotes toggle quoting and are
// dropped wherever they stand, a delimiter inside quotes belongs to the cell, '\r' is dropped, zero-length lines are skipped,
// short records are padded with NULLs and long ones cut — what the line-by-line reader this replaces did (0.055 GB/s: one
// std::string per cell, every cell parsed three times with strtod).
namespace csv {

struct Text {
    std::string buf;                                   // the file image
    std::vector<std::pair<size_t, size_t>> records;    // [begin, end) of every data record
    std::vector<std::string> header;
    char delimiter = ',';
};
struct Cell { const char* b; const char* e; bool dirty; };   // dirty: holds quotes or '\r' that are not part of the value

// the cells of one record, at most `ncols` of them (missing ones come back empty)
inline void split(const char* b, const char* e, char delimiter, size_t ncols, Cell* out) {
    size_t c = 0;
    bool q = false, dirty = false;
    const char* start = b;
    for (const char* p = b; p < e && c < ncols; ++p) {
        if (*p == '"') { q = !q; dirty = true; }
        else if (*p == '\r') dirty = true;
        else if (*p == delimiter && !q) { out[c++] = Cell{start, p, dirty}; start = p + 1; dirty = false; }
    }
    if (c < ncols) {
        const char* end = e;
        bool d = false;
        for (const char* p = start; p < e; ++p) {
            if (*p == '"') { q = !q; d = true; } else if (*p == '\r') d = true; else if (*p == delimiter && !q) { end = p; break; }
        }
        out[c++] = Cell{start, end, d};
    }
    for (; c < ncols; ++c) out[c] = Cell{e, e, false};
}
inline std::string cell_text(const Cell& c) {
    std::string t;
    t.reserve((size_t)(c.e - c.b));
    for (const char* p = c.b; p < c.e; ++p) if (*p != '"' && *p != '\r') t += *p;
    return t;
}
inline const char* skip_lead(const char* b, const char* e, bool* ok) {   // strtoll / strtod take leading blanks and one '+'
    while (b < e && (*b == ' ' || *b == '\t')) ++b;
    if (b < e && *b == '+') { ++b; if (b < e && (*b == '+' || *b == '-')) *ok = false; }
    if (b == e) *ok = false;
    return b;
}
inline bool parse_i64(const char* b, const char* e, int64_t& v) {
    bool ok = true;
    b = skip_lead(b, e, &ok);
    if (!ok) return false;
    const auto r = std::from_chars(b, e, v, 10);
    return r.ec == std::errc() && r.ptr == e;
}
inline bool parse_f64(const char* b, const char* e, double& v) {
    bool ok = true;
    b = skip_lead(b, e, &ok);
    if (!ok) return false;
    const auto r = std::from_chars(b, e, v);
    if (r.ec == std::errc() && r.ptr == e) return true;
    const std::string t(b, e);                          // what strtod takes and from_chars does not (hex floats, overflow to inf)
    char* end = nullptr;
    v = std::strtod(t.c_str(), &end);
    return end != t.c_str() && !*end;
}
inline bool is_bool(const char* b, const char* e, bool* value = nullptr) {
    const size_t n = (size_t)(e - b);
    auto eq = [&](const char* w) { return std::strlen(w) == n && std::memcmp(b, w, n) == 0; };
    if (eq("true") || eq("True") || eq("TRUE")) { if (value) *value = true; return true; }
    if (eq("false") || eq("False") || eq("FALSE")) { if (value) *value = false; return true; }
    return false;
}

inline Text load(const std::string& path, bool has_headers = true, char delimiter = ',', std::optional<size_t> max_records = std::nullopt) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw DataFrameError(DataFrameError::IoError, "cannot open " + path);
    Text t;
    t.delimiter = delimiter;
    const std::streamoff size = f.tellg();
    f.seekg(0);
    t.buf.resize((size_t)size);
    if (size > 0 && !f.read(&t.buf[0], size)) throw DataFrameError(DataFrameError::IoError, "cannot read " + path);
    const char* base = t.buf.data();
    const char* end = base + t.buf.size();
    // the header: the first line that is not empty (or, without a header row, just its number of cells)
    const char* p = base;
    while (p < end) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        if (le > p) {
            size_t ncols = 1;
            { bool q = false; for (const char* c = p; c < le; ++c) { if (*c == '"') q = !q; else if (*c == delimiter && !q) ++ncols; } }
            std::vector<Cell> cells(ncols);
            split(p, le, delimiter, ncols, cells.data());
            if (has_headers) { for (auto& c : cells) t.header.push_back(cell_text(c)); p = nl ? nl + 1 : end; }
            else for (size_t i = 0; i < ncols; ++i) t.header.push_back("column_" + std::to_string(i + 1));   // arrow's csv reader names
            break;
        }
        p = nl ? nl + 1 : end;
    }
    // the records: [begin, end) of every line that is not empty.  A long file is cut into byte ranges, one thread each; a thread
    // takes the lines that START in its range (it finds its first line start behind the first '\n' at or after the range's
    // begin - 1) and follows its last line past the range's end.
    const char* body = p;
    auto scan = [&](const char* from, const char* upto, std::vector<std::pair<size_t, size_t>>& out, size_t stop_after) {
        const char* q = from;
        while (q < upto && out.size() < stop_after) {
            const char* nl = (const char*)std::memchr(q, '\n', (size_t)(end - q));
            const char* le = nl ? nl : end;
            if (le > q) out.emplace_back((size_t)(q - base), (size_t)(le - base));
            q = nl ? nl + 1 : end;
        }
    };
    const size_t limit = max_records ? *max_records : (size_t)-1;
    const size_t bytes = (size_t)(end - body);
    const int T = (int)std::min<size_t>({(size_t)std::max(1u, std::thread::hardware_concurrency()), (size_t)16, bytes / ((size_t)4 << 20) + 1});
    if (T <= 1 || max_records) scan(body, end, t.records, limit);
    else {
        std::vector<std::vector<std::pair<size_t, size_t>>> part((size_t)T);
        std::vector<std::thread> pool;
        for (int w = 0; w < T; ++w)
            pool.emplace_back([&, w]() {
                const char* b = body + bytes * (size_t)w / (size_t)T;
                const char* e = body + bytes * (size_t)(w + 1) / (size_t)T;
                if (w > 0) {   // the first line start at or behind b: one past the first '\n' at or behind b - 1
                    const char* nl = (const char*)std::memchr(b - 1, '\n', (size_t)(end - (b - 1)));
                    b = nl ? nl + 1 : end;
                }
                scan(b, e, part[(size_t)w], (size_t)-1);
            });
        for (auto& th : pool) th.join();
        size_t total = 0;
        for (auto& v : part) total += v.size();
        t.records.reserve(total);
        for (auto& v : part) t.records.insert(t.records.end(), v.begin(), v.end());
    }
    return t;
}

// worker threads over ranges of records that start on multiples of 64 (validity bytes and words are never shared)
template <class F>
inline void for_ranges(size_t n, int threads, F&& body) {
    int T = threads > 0 ? threads : (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
    const size_t per = ((n + (size_t)T - 1) / (size_t)T + 63) / 64 * 64;
    if (n < 32768 || T == 1) { body(0, (size_t)0, n); return; }
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> errs((size_t)T);
    int t = 0;
    for (size_t r0 = 0; r0 < n; r0 += per, ++t)
        pool.emplace_back([&, t, r0]() { try { body(t, r0, std::min(n, r0 + per)); } catch (...) { errs[(size_t)t] = std::current_exception(); } });
    for (auto& th : pool) th.join();
    for (auto& e : errs) if (e) std::rethrow_exception(e);
}
inline int range_count(size_t n, int threads) {
    int T = threads > 0 ? threads : (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
    if (n < 32768 || T == 1) return 1;
    const size_t per = ((n + (size_t)T - 1) / (size_t)T + 63) / 64 * 64;
    return (int)((n + per - 1) / per);
}

struct Inferred { DataType dtype = DataType::Utf8; bool any_null = false, any = false; };   // any: some cell of the column is not empty
// the types of the columns `cols` (indices into the header), from the first `limit` records
inline std::vector<Inferred> infer(const Text& t, const std::vector<size_t>& cols, int threads = 0, size_t limit = (size_t)-1) {
    struct Flags { bool all_int = true, all_num = true, all_bool = true, any = false, nulls = false; };
    const size_t nh = t.header.size(), n = std::min(t.records.size(), limit);
    const int nr = range_count(n, threads);
    std::vector<std::vector<Flags>> part((size_t)nr, std::vector<Flags>(cols.size()));
    for_ranges(n, threads, [&](int w, size_t r0, size_t r1) {
        std::vector<Cell> cells(nh);
        std::vector<Flags>& fl = part[(size_t)w];
        for (size_t r = r0; r < r1; ++r) {
            split(t.buf.data() + t.records[r].first, t.buf.data() + t.records[r].second, t.delimiter, nh, cells.data());
            for (size_t k = 0; k < cols.size(); ++k) {
                Cell c = cells[cols[k]];
                std::string clean;
                if (c.dirty) { clean = cell_text(c); c = Cell{clean.data(), clean.data() + clean.size(), false}; }
                Flags& f = fl[k];
                if (c.b == c.e) { f.nulls = true; continue; }
                f.any = true;
                int64_t iv; double dv;
                if (f.all_int && !parse_i64(c.b, c.e, iv)) f.all_int = false;
                if (!f.all_int && f.all_num && !parse_f64(c.b, c.e, dv)) f.all_num = false;
                if (f.all_bool && !is_bool(c.b, c.e)) f.all_bool = false;
            }
        }
    });
    std::vector<Inferred> out(cols.size());
    for (size_t k = 0; k < cols.size(); ++k) {
        Flags m;
        for (auto& p : part) { m.all_int &= p[k].all_int; m.all_num &= p[k].all_num; m.all_bool &= p[k].all_bool; m.any |= p[k].any; m.nulls |= p[k].nulls; }
        // (a range that met no cell that breaks "integer" never tried "number": an integer is a number)
        out[k].any_null = m.nulls;
        out[k].any = m.any;
        out[k].dtype = !m.any ? DataType::Utf8 : m.all_int ? DataType::Int64 : m.all_num ? DataType::Float64 : m.all_bool ? DataType::Boolean : DataType::Utf8;
    }
    return out;
}

struct Filled { int64_t nulls = 0; std::vector<std::string> strings; };   // strings: the cells of a Utf8 column
// Parse column cols[k] of every record into values[k] (8 bytes per row; Boolean: one bit per row) and validity[k] (one bit per
// row, 1 = valid); both zeroed here.  Utf8 columns (values[k] == nullptr) come back as strings.
// `violated` (optional, one flag per column): a non-empty cell did not parse as the column's type — the types came from a sample
// of the records and the caller has to infer them from all of them after all.
inline std::vector<Filled> fill(const Text& t, const std::vector<size_t>& cols, const std::vector<Inferred>& types,
                                const std::vector<uint8_t*>& values, const std::vector<uint8_t*>& validity, int threads = 0,
                                std::vector<char>* violated = nullptr) {
    const size_t nh = t.header.size(), n = t.records.size();
    std::vector<Filled> out(cols.size());
    for (size_t k = 0; k < cols.size(); ++k) {
        if (types[k].dtype == DataType::Utf8) { out[k].strings.resize(n); continue; }
        std::memset(values[k], 0, types[k].dtype == DataType::Boolean ? (n + 7) / 8 : n * 8);
        std::memset(validity[k], 0, (n + 7) / 8);
    }
    const int nr = range_count(n, threads);
    std::vector<std::vector<int64_t>> nulls((size_t)nr, std::vector<int64_t>(cols.size(), 0));
    for_ranges(n, threads, [&](int w, size_t r0, size_t r1) {
        std::vector<Cell> cells(nh);
        for (size_t r = r0; r < r1; ++r) {
            split(t.buf.data() + t.records[r].first, t.buf.data() + t.records[r].second, t.delimiter, nh, cells.data());
            for (size_t k = 0; k < cols.size(); ++k) {
                Cell c = cells[cols[k]];
                std::string clean;
                if (c.dirty) { clean = cell_text(c); c = Cell{clean.data(), clean.data() + clean.size(), false}; }
                const DataType dt = types[k].dtype;
                if (dt == DataType::Utf8) { out[k].strings[r].assign(c.b, c.e); continue; }
                if (c.b == c.e) { ++nulls[(size_t)w][k]; continue; }
                validity[k][r >> 3] |= (uint8_t)(1u << (r & 7));
                bool ok;
                if (dt == DataType::Int64) { int64_t v = 0; ok = parse_i64(c.b, c.e, v); std::memcpy(values[k] + 8 * r, &v, 8); }
                else if (dt == DataType::Float64) { double v = 0; ok = parse_f64(c.b, c.e, v); std::memcpy(values[k] + 8 * r, &v, 8); }
                else { bool v = false; ok = is_bool(c.b, c.e, &v); if (v) values[k][r >> 3] |= (uint8_t)(1u << (r & 7)); }
                if (!ok && violated) (*violated)[k] = 1;     // (a racing store of the same value from several threads)
            }
        }
    });
    for (size_t k = 0; k < cols.size(); ++k) for (auto& p : nulls) out[k].nulls += p[k];
    return out;
}

}  // namespace csv

namespace plan {

struct Column {  // expression::Column {name, column_type: Scalar(dtype)}
    std::string name;
    DataType data_type;
    std::string debug() const { return "Column { name: \"" + name + "\", column_type: Scalar(" + type_name(data_type) + ") }"; }
};
struct Dataset {
    std::string name;
    std::vector<Column> columns;
    std::optional<std::pair<size_t, Column>> get_column(const std::string& n) const {
        for (size_t i = 0; i < columns.size(); ++i) if (columns[i].name == n) return std::make_pair(i, columns[i]);
        return std::nullopt;
    }
    Dataset append_column(const Column& c) const {  // :95-112: replace in place or push
        Dataset d = *this;
        for (auto& e : d.columns) if (e.name == c.name) { e = c; return d; }
        d.columns.push_back(c);
        return d;
    }
};
enum class ScalarFunction { Add, Subtract, Divide, Multiply, Abs, Sine, Cosine, Tangent, Cotangent, Secant, Cosecant };
inline const char* scalar_function_name(ScalarFunction f) {
    static const char* n[] = {"Add", "Subtract", "Divide", "Multiply", "Abs", "Sine", "Cosine", "Tangent", "Cotangent", "Secant", "Cosecant"};
    return n[(int)f];
}
enum class AggregateFunction { Avg, Count, CountDistinct, First, Kurtosis, Last, Max, Min, Skewness, StdDev, Sum, SumDistinct, Variance };
struct Function {
    enum Kind { Scalar, Cast, Rename, Filter } kind = Scalar;
    ScalarFunction scalar = ScalarFunction::Add;
    FilterRef filter;
    static Function Scalar_(ScalarFunction f) { Function x; x.kind = Scalar; x.scalar = f; return x; }
    static Function Cast_() { Function x; x.kind = Cast; return x; }
    static Function Rename_() { Function x; x.kind = Rename; return x; }
    static Function Filter_(FilterRef f) { Function x; x.kind = Filter; x.filter = std::move(f); return x; }
    std::string debug() const {
        switch (kind) { case Cast: return "Cast"; case Rename: return "Rename"; case Filter: return "Filter(..)";
                        default: return std::string("Scalar(") + scalar_function_name(scalar) + ")"; }
    }
};
struct Calculation {
    std::string name;
    std::vector<Column> inputs;
    Column output;
    Function function;
    std::string debug() const {  // mirrors #[derive(Debug)] so the reference's plan-text test can be restated
        std::string s = "Calculation { name: \"" + name + "\", inputs: [";
        for (size_t i = 0; i < inputs.size(); ++i) s += (i ? ", " : "") + inputs[i].debug();
        return s + "], output: " + output.debug() + ", function: " + function.debug() + " }";
    }
};
inline std::string debug(const std::vector<Calculation>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + v[i].debug();
    return s + "]";
}
struct Aggregation { AggregateFunction function; std::vector<std::string> columns; };

// Dataset::try_aggregate (src/expression.rs:114-221): the planned output of GroupAggregate — the grouping columns, then one
// column per (aggregation, input column) named "avg(x)" / "sum(x)" / "max(x)" / "min(x)" / "count(x)" / "count_distinct(x)"
// / "first(x)" / "last(x)", typed like the input except the counts (UInt32); the remaining functions are
// "Aggregation not yet supported".  (The reference PLANS avg with the input's type; evaluated, an average is Float64 —
// AggregateFunctions::avg, src/functions/aggregate.rs:32.)
inline Dataset try_aggregate(const Dataset& self, const std::vector<std::string>& groups, const std::vector<Aggregation>& aggr) {
    Dataset out;
    out.name = "aggregated_dataset";
    for (auto& g : groups) {
        const auto c = self.get_column(g);
        if (!c) throw DataFrameError(DataFrameError::ComputeError, "Grouping column \"" + g + "\" does not exist");
        out.columns.push_back(c->second);
    }
    for (auto& a : aggr)
        for (auto& name : a.columns) {
            const auto c = self.get_column(name);
            if (!c) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column \"" + name + "\" does not exist");
            const DataType t = c->second.data_type;
            switch (a.function) {
                case AggregateFunction::Avg: out.columns.push_back(Column{"avg(" + name + ")", t}); break;
                case AggregateFunction::Sum: out.columns.push_back(Column{"sum(" + name + ")", t}); break;
                case AggregateFunction::Max: out.columns.push_back(Column{"max(" + name + ")", t}); break;
                case AggregateFunction::Min: out.columns.push_back(Column{"min(" + name + ")", t}); break;
                case AggregateFunction::Count: out.columns.push_back(Column{"count(" + name + ")", DataType::UInt32}); break;
                case AggregateFunction::CountDistinct: out.columns.push_back(Column{"count_distinct(" + name + ")", DataType::UInt32}); break;
                case AggregateFunction::First: out.columns.push_back(Column{"first(" + name + ")", t}); break;
                case AggregateFunction::Last: out.columns.push_back(Column{"last(" + name + ")", t}); break;
                default: throw DataFrameError(DataFrameError::ComputeError, "Aggregation not yet supported");
            }
        }
    return out;
}

// Dataset::try_join (src/expression.rs:223-285): both key columns must exist and have the same type; the output holds the
// columns of both sides, a name present on both sides as "a.<name>" / "b.<name>"
inline Dataset try_join(const Dataset& a, const Dataset& b, const std::vector<std::pair<std::string, std::string>>& on) {
    for (auto& c : on) {
        const auto ca = a.get_column(c.first), cb = b.get_column(c.second);
        if (ca && cb) { if (ca->second.data_type != cb->second.data_type) throw DataFrameError(DataFrameError::ComputeError, "Join columns must have compatible types"); }
        else if (!ca && cb) throw DataFrameError(DataFrameError::ComputeError, "Join column does not exist in table A");
        else if (ca && !cb) throw DataFrameError(DataFrameError::ComputeError, "Join column does not exist in table B");
        else throw DataFrameError(DataFrameError::ComputeError, "Join columns do not exist in tables");
    }
    Dataset out;
    out.name = "joined_dataframe";
    for (auto& c : a.columns) out.columns.push_back(b.get_column(c.name) ? Column{"a." + c.name, c.data_type} : c);
    for (auto& c : b.columns) out.columns.push_back(a.get_column(c.name) ? Column{"b." + c.name, c.data_type} : c);
    return out;
}

struct ArrowError : DataFrameError { using DataFrameError::DataFrameError; };

// CastOperation (src/operation/scalar.rs:95-137)
struct CastOperation {
    static const char* name() { return "cast"; }
    static std::vector<Calculation> transform(const std::vector<Column>& inputs, std::optional<std::string> out_name, std::optional<DataType> to_type) {
        if (inputs.size() != 1) throw DataFrameError(DataFrameError::ComputeError, "Cast operation expects 1 input");
        if (!to_type) throw DataFrameError(DataFrameError::ArrowError, "Cast requires a target output datatype");
        const Column& a = inputs[0];
        return {Calculation{name(), inputs, Column{out_name.value_or(std::string(name()) + "(" + a.name + " as datatype)"), *to_type}, Function::Cast_()}};
    }
};
// AddOperation / SubtractOperation (:18-93, :139-214) + the same shape for multiply / divide
template <ScalarFunction F>
struct BinaryOperation {
    static const char* name() {
        return F == ScalarFunction::Add ? "add" : F == ScalarFunction::Subtract ? "subtract" : F == ScalarFunction::Multiply ? "multiply" : "divide";
    }
    static std::vector<Calculation> transform(const std::vector<Column>& inputs, std::optional<std::string> out_name, std::optional<DataType>) {
        if (inputs.size() != 2) throw DataFrameError(DataFrameError::ComputeError, std::string(name()) + " operation expects 2 inputs");
        const Column &a = inputs[0], &b = inputs[1];
        const std::string oname = out_name.value_or(std::string(name()) + "(" + a.name + ", " + b.name + ")");
        if (a.data_type != b.data_type) {
            // cast b to a's type first (:47-72).  The reference's subtract emits Add here: not copied.
            auto cast = CastOperation::transform({b}, b.name, a.data_type)[0];
            return {cast, Calculation{name(), {a, cast.output}, Column{oname, a.data_type}, Function::Scalar_(F)}};
        }
        return {Calculation{name(), inputs, Column{oname, a.data_type}, Function::Scalar_(F)}};
    }
};
using AddOperation = BinaryOperation<ScalarFunction::Add>;
using SubtractOperation = BinaryOperation<ScalarFunction::Subtract>;
using MultiplyOperation = BinaryOperation<ScalarFunction::Multiply>;
using DivideOperation = BinaryOperation<ScalarFunction::Divide>;
// SinOperation (:227-318) + the same shape for cosine / tangent: integers are cast to Float64 first
template <ScalarFunction F>
struct TrigOperation {
    static const char* name() {
        return F == ScalarFunction::Sine ? "sin" : F == ScalarFunction::Cosine ? "cos" : F == ScalarFunction::Tangent ? "tan"
             : F == ScalarFunction::Cotangent ? "cot" : F == ScalarFunction::Secant ? "sec" : "csc";
    }
    static std::vector<Calculation> transform(const std::vector<Column>& inputs, std::optional<std::string> out_name, std::optional<DataType>) {
        if (inputs.size() != 1) throw DataFrameError(DataFrameError::ComputeError, "Sine operation expects 2 inputs");  // sic, :242
        const Column& a = inputs[0];
        const std::string oname = out_name.value_or(std::string(name()) + "(" + a.name + " as datatype)");
        if (is_integer(a.data_type)) {
            const Column cast_out{out_name.value_or(std::string(CastOperation::name()) + "(" + a.name + " as datatype)"), DataType::Float64};
            return {Calculation{CastOperation::name(), inputs, cast_out, Function::Cast_()},
                    Calculation{name(), {cast_out}, Column{oname, DataType::Float64}, Function::Scalar_(F)}};
        }
        if (is_float(a.data_type)) return {Calculation{name(), inputs, Column{oname, a.data_type}, Function::Scalar_(F)}};
        throw DataFrameError(DataFrameError::ComputeError, std::string("Cannot perform ") + name() + " operation from " + type_name(a.data_type) + " data type");
    }
};
using SinOperation = TrigOperation<ScalarFunction::Sine>;
using CosOperation = TrigOperation<ScalarFunction::Cosine>;
using TanOperation = TrigOperation<ScalarFunction::Tangent>;
// ScalarFunction::{Cotangent, Secant, Cosecant} (:670-672): the reference's builder panics on them (:487-489); planned
// here with the sine's shape and evaluated as RDF_OP_COT / SEC / CSC
using CotOperation = TrigOperation<ScalarFunction::Cotangent>;
using SecOperation = TrigOperation<ScalarFunction::Secant>;
using CscOperation = TrigOperation<ScalarFunction::Cosecant>;

// Reader / DataSourceType / CsvReadOptions (src/expression.rs:344-378): where a plan's rows come from.  CSV and Arrow IPC are the
// sources this mirror loads (the others are IO outside the hot path); the CSV options are what the optimiser pushes into.
struct CsvReadOptions {
    bool has_headers = true;
    std::optional<uint8_t> delimiter;
    std::optional<size_t> max_records;
    size_t batch_size = 1024;
    std::optional<std::vector<size_t>> projection;
};
struct Reader {
    enum Source { Csv, Json, Arrow, Sql, Parquet } source = Csv;
    std::string path;
    CsvReadOptions csv;
    static Reader Csv_(std::string p, CsvReadOptions o = CsvReadOptions()) { Reader r; r.source = Csv; r.path = std::move(p); r.csv = std::move(o); return r; }
    static Reader Arrow_(std::string p) { Reader r; r.source = Arrow; r.path = std::move(p); return r; }
    // Reader::get_dataset: the schema the source will produce (CSV: inferred from the text, host only)
    Dataset get_dataset() const {
        if (source != Csv) throw DataFrameError(DataFrameError::ComputeError, "get_dataset: only CSV sources are planned here");
        const csv::Text t = csv::load(path, csv.has_headers, (char)csv.delimiter.value_or((uint8_t)','), csv.max_records);
        std::vector<size_t> cols;
        for (size_t i = 0; i < t.header.size(); ++i)
            if (!csv.projection || std::find(csv.projection->begin(), csv.projection->end(), i) != csv.projection->end()) cols.push_back(i);
        const std::vector<csv::Inferred> types = csv::infer(t, cols);
        Dataset d;
        d.name = "csv_source";
        for (size_t k = 0; k < cols.size(); ++k) d.columns.push_back(Column{t.header[cols[k]], types[k].dtype});
        return d;
    }
};

struct Transformation {
    enum Kind { GroupAggregate, Calculate, Select, Drop, Limit, Filter, Sort, Join, Read } kind = Calculate;
    Reader reader;                          // Read
    Calculation calc;                       // Calculate
    std::vector<std::string> names;         // Select / Drop / group columns
    std::vector<Aggregation> aggregations;  // GroupAggregate
    size_t limit = 0;
    FilterRef filter;
    std::vector<bool> sort_descending;      // Sort: per criterion (names holds the columns)
    static Transformation Read_(Reader r) { Transformation t; t.kind = Read; t.reader = std::move(r); return t; }
    static Transformation Calculate_(Calculation c) { Transformation t; t.kind = Calculate; t.calc = std::move(c); return t; }
    static Transformation Filter_(FilterRef f) { Transformation t; t.kind = Filter; t.filter = std::move(f); return t; }
    static Transformation Limit_(size_t n) { Transformation t; t.kind = Limit; t.limit = n; return t; }
    static Transformation Select_(std::vector<std::string> n) { Transformation t; t.kind = Select; t.names = std::move(n); return t; }
    static Transformation Drop_(std::vector<std::string> n) { Transformation t; t.kind = Drop; t.names = std::move(n); return t; }
    static Transformation Sort_(std::vector<std::string> cols, std::vector<bool> descending) {
        Transformation t; t.kind = Sort; t.names = std::move(cols); t.sort_descending = std::move(descending); return t;
    }
    static Transformation GroupAggregate_(std::vector<std::string> groups, std::vector<Aggregation> a) {
        Transformation t; t.kind = GroupAggregate; t.names = std::move(groups); t.aggregations = std::move(a); return t;
    }
};
struct Computation {
    std::vector<Dataset> input;
    std::vector<Transformation> transformations;
    Dataset output;
    static Computation empty() { return Computation(); }
    // Computation::compute_read (src/expression.rs:571-578)
    static Computation compute_read(const Reader& read) {
        Computation c;
        c.transformations = {Transformation::Read_(read)};
        c.output = read.get_dataset();
        return c;
    }
    bool is_single(Transformation::Kind k) const { return transformations.size() == 1 && transformations[0].kind == k; }
};

// optimise (src/optimiser.rs:5-101) over an unrolled plan (newest computation first, the read last), with its two helpers
// (:103-181 optimise_read, :183-235 optimise_project_calc).  The same rules: two Limits merge into the smaller; a Limit sinks
// below the computation that follows it; a Select / Limit in front of a CSV Read becomes the reader's projection /
// max_records; a Select that names a computed column and all of its inputs is pushed above the Calculate, a Calculate whose
// output is not selected is dropped.  Deliberate differences (intent reproduced, bugs not copied — this plan is evaluated, the
// reference's is only printed): the projection indices are taken against the READ's columns (the reference enumerates the
// Select's own output, right only while the selected columns are a prefix of the file's); the computation still pending when
// the list ends is emitted (the reference returns without it unless optimise_read happened to emit it: [Calculate, Read] comes
// back as [Calculate]); and where the reference's optimise_project_calc says "drop calculation" it returns the calculation and
// drops the SELECT (its `project` argument is the calculate computation) — here the calculation goes and the select stays.
inline std::pair<std::vector<Computation>, Computation> optimise_read(const Computation& input, const Computation& read, const Transformation& x, bool* emitted) {
    std::vector<Computation> output;
    Computation mutated = read;
    const Reader& reader = read.transformations[0].reader;
    *emitted = false;
    if (reader.source != Reader::Csv) { output.push_back(input); return {output, mutated}; }   // no projection support (Arrow / Json / Parquet / Sql)
    CsvReadOptions options = reader.csv;
    if (x.kind == Transformation::Select && !options.projection) {
        std::vector<size_t> proj;
        Dataset out_ds;
        out_ds.name = read.output.name;
        for (size_t i = 0; i < read.output.columns.size(); ++i)
            if (std::find(x.names.begin(), x.names.end(), read.output.columns[i].name) != x.names.end()) { proj.push_back(i); out_ds.columns.push_back(read.output.columns[i]); }
        options.projection = proj;
        mutated.transformations = {Transformation::Read_(Reader::Csv_(reader.path, options))};
        mutated.output = out_ds;
        output.push_back(mutated);
        *emitted = true;
    } else if (x.kind == Transformation::Limit) {
        options.max_records = options.max_records ? std::min(*options.max_records, x.limit) : x.limit;
        mutated.transformations = {Transformation::Read_(Reader::Csv_(reader.path, options))};
        output.push_back(mutated);
        *emitted = true;
    } else {
        output.push_back(input);   // Drop, a second projection, anything else: kept as it is
    }
    return {output, mutated};
}
inline std::pair<std::vector<Computation>, Computation> optimise_project_calc(const Computation& input, const Computation& project, const Transformation& x, const Calculation& calc) {
    std::vector<Computation> output;
    Computation mutated = project;
    if (x.kind == Transformation::Select) {
        const bool selected_output = std::find(x.names.begin(), x.names.end(), calc.output.name) != x.names.end();
        if (!selected_output) return {output, input};     // the calculated column is not selected: the calculation is dropped, the select stays pending
        size_t selected_inputs = 0;
        for (auto& in : calc.inputs) selected_inputs += std::find(x.names.begin(), x.names.end(), in.name) != x.names.end();
        if (selected_inputs == calc.inputs.size()) {     // every input is selected: the select moves above the calculation
            output.push_back(input);
            Dataset d;
            d.name = mutated.output.name;
            for (auto& c : mutated.output.columns) if (c.name != calc.output.name) d.columns.push_back(c);
            mutated.output = d;
            return {output, mutated};
        }
        output.push_back(input);   // an input of the calculation is not selected: both steps stay as they are
    } else {
        output.push_back(input);   // Drop
    }
    return {output, mutated};
}
inline std::vector<Computation> optimise(const std::vector<Computation>& computations) {
    std::vector<Computation> output;
    Computation input = Computation::empty();
    bool pending = false;   // `input` holds a computation that is not in `output` yet
    auto emit = [&](const Computation& c) { output.push_back(c); };
    for (const Computation& c : computations) {
        if (input.transformations.empty()) { input = c; pending = true; continue; }
        const size_t ci = c.input.size(), ii = input.input.size();
        if (ci == 0 && ii == 1 && c.is_single(Transformation::Read) && input.transformations.size() == 1) {
            bool emitted = false;
            auto r = optimise_read(input, c, input.transformations[0], &emitted);
            for (auto& o : r.first) emit(o);
            input = r.second;
            pending = !emitted;
        } else if (ci == 1 && ii == 1 && input.is_single(Transformation::Limit) && c.is_single(Transformation::Limit)) {
            input.transformations = {Transformation::Limit_(std::min(input.transformations[0].limit, c.transformations[0].limit))};
            emit(input);
            pending = false;
        } else if (ci == 1 && ii == 1 && input.is_single(Transformation::Limit) && !c.is_single(Transformation::Limit)) {
            emit(c);               // the limit sinks below the computation that follows it; it stays the pending input
        } else if (ci == 1 && ii == 1 && (input.is_single(Transformation::Select) || input.is_single(Transformation::Drop)) && c.is_single(Transformation::Calculate)) {
            auto r = optimise_project_calc(input, c, input.transformations[0], c.transformations[0].calc);
            for (auto& o : r.first) emit(o);
            input = r.second;
            pending = true;
        } else {
            if (pending) emit(input);
            input = c;
            pending = true;
        }
    }
    if (pending && !input.transformations.empty()) emit(input);
    return output;
}

// Calculation::calculate (src/expression.rs:433-499): name lookup + dispatch to the operation builders.
inline std::vector<Transformation> calculate(const Dataset& ds, const std::vector<std::string>& in_col_names, const Function& function,
                                             std::optional<std::string> out_col_name, std::optional<DataType> out_col_type) {
    std::vector<Column> inputs;
    for (auto& n : in_col_names) {
        auto c = ds.get_column(n);
        if (!c) throw DataFrameError(DataFrameError::ParseError, "Column " + n + " not found");
        inputs.push_back(c->second);
    }
    std::vector<Calculation> ops;
    switch (function.kind) {
        case Function::Filter: return {Transformation::Filter_(function.filter)};
        case Function::Cast: ops = CastOperation::transform(inputs, out_col_name, out_col_type); break;
        case Function::Rename: throw DataFrameError(DataFrameError::ComputeError, "Please use rename function directly for now");
        default:
            switch (function.scalar) {
                case ScalarFunction::Add: ops = AddOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Subtract: ops = SubtractOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Multiply: ops = MultiplyOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Divide: ops = DivideOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Sine: ops = SinOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Cosine: ops = CosOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Tangent: ops = TanOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Cotangent: ops = CotOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Secant: ops = SecOperation::transform(inputs, out_col_name, out_col_type); break;
                case ScalarFunction::Cosecant: ops = CscOperation::transform(inputs, out_col_name, out_col_type); break;
                default: throw DataFrameError(DataFrameError::ComputeError, std::string("Scalar Function ") + scalar_function_name(function.scalar) + " not supported");
            }
    }
    std::vector<Transformation> out;
    for (auto& c : ops) out.push_back(Transformation::Calculate_(c));
    return out;
}

}  // namespace plan

// ------------------------------------------------------------------------------------------------
// DataFrame (src/dataframe.rs:30-337)

struct RecordBatch {
    Schema schema;
    std::vector<ArrayRef> columns;
    int64_t num_rows() const { return columns.empty() ? 0 : columns[0]->length; }
};

// arrow::compute::cast per chunk (Function::Cast, src/evaluation.rs:296-315) on device arrays
inline std::vector<ArrayRef> cast_arrays(const std::vector<ArrayRef>& arr, DataType to) {
    std::vector<rdf_array> a;
    std::vector<std::shared_ptr<Array>> outs;
    std::vector<rdf_out> ov;
    for (auto& x : arr) { a.push_back(x->view()); outs.push_back(Array::make_out(to, x->length, true, x->host)); ov.push_back(outs.back()->out_view(x->length)); }   // (a value the target type cannot hold becomes NULL: always a bitmap)
    check(rdf_cast(a.data(), (int64_t)a.size(), ov.data()));
    std::vector<ArrayRef> res;
    for (size_t i = 0; i < outs.size(); ++i) { outs[i]->length = ov[i].length; outs[i]->null_count = ov[i].null_count; res.push_back(outs[i]); }
    return res;
}

// Minimal in-place flatbuffer reader for the Arrow IPC metadata (tables via vtables, vectors, strings, structs);
// every access is bounds-checked against the file image.
struct FlatBuf {
    const uint8_t* base; size_t size;
    [[noreturn]] static void oob() { throw DataFrameError(DataFrameError::IoError, "Arrow IPC: metadata out of bounds"); }
    template <class T> T rd(size_t pos) const { if (pos + sizeof(T) > size) oob(); T v; std::memcpy(&v, base + pos, sizeof(T)); return v; }
    size_t root(size_t pos) const { return pos + rd<uint32_t>(pos); }                 // position of the root table
    // position of field `id` inside table `t`, or 0 when absent (default value)
    size_t field_pos(size_t t, int id) const {
        if (!t) return 0;
        const int32_t so = rd<int32_t>(t);
        const size_t vt = (size_t)((int64_t)t - so);
        const uint16_t vsize = rd<uint16_t>(vt);
        const size_t slot = 4 + 2 * (size_t)id;
        if (slot + 2 > vsize) return 0;
        const uint16_t off = rd<uint16_t>(vt + slot);
        return off ? t + off : 0;
    }
    template <class T> T scalar(size_t t, int id, T def) const { const size_t p = field_pos(t, id); return p ? rd<T>(p) : def; }
    size_t table_field(size_t t, int id) const { const size_t p = field_pos(t, id); return p ? p + rd<uint32_t>(p) : 0; }
    std::string string(size_t t, int id) const {
        const size_t p = field_pos(t, id);
        if (!p) return "";
        const size_t s = p + rd<uint32_t>(p);
        const uint32_t n = rd<uint32_t>(s);
        if (s + 4 + n > size) oob();
        return std::string((const char*)base + s + 4, n);
    }
    // `fp` = position of a vector FIELD (from field_pos), 0 = absent
    size_t vec_len(size_t fp) const { return fp ? rd<uint32_t>(fp + rd<uint32_t>(fp)) : 0; }
    size_t vec_table(size_t fp, size_t i) const { const size_t e = fp + rd<uint32_t>(fp) + 4 + 4 * i; return e + rd<uint32_t>(e); }
    const uint8_t* vec_struct(size_t fp, size_t i, size_t stride) const {
        const size_t e = fp + rd<uint32_t>(fp) + 4 + stride * i;
        if (e + stride > size) oob();
        return base + e;
    }
};

class DataFrame {
  public:
    DataFrame() = default;
    DataFrame(Schema schema, std::vector<Column> columns) : schema_(std::move(schema)), columns_(std::move(columns)) {}
    static DataFrame empty() { return DataFrame(); }
    static DataFrame from_columns(std::vector<Column> cols) {
        Schema s;
        for (auto& c : cols) s.fields.push_back(c.field());
        for (auto& c : cols)
            if (c.num_rows() != cols[0].num_rows()) throw DataFrameError(DataFrameError::ComputeError, "columns differ in length");
        return DataFrame(std::move(s), std::move(cols));
    }
    // DataFrame::from_csv (src/dataframe.rs:349-389: arrow::csv::Reader with an inferred schema, batch_size 1024).
    // Schema inference as the Arrow CSV reader does it — a column whose non-empty cells all parse as integers is Int64,
    // as numbers Float64, as true / false Boolean, anything else Utf8; an empty cell is a NULL.  A typed column is parsed
    // into ONE host buffer (+ validity bitmap) and reaches HBM with ONE copy; its 1024-row RecordBatches are zero-copy
    // slices of that buffer (chunk i = offset 1024 i), so the chunk structure the reference's reader produces is kept
    // without one small copy per batch.  Quoted text columns are carried as opaque Utf8 on the host.
    static DataFrame from_csv(const std::string& path, size_t batch_size = 1024) {
        plan::CsvReadOptions o;
        o.batch_size = batch_size;
        return from_csv(path, o);
    }
    // ... with the reader's options (src/expression.rs:372-378): header row, delimiter, max_records, batch_size, projection —
    // what plan::optimise pushes a Limit / Select into
    static DataFrame from_csv(const std::string& path, const plan::CsvReadOptions& options) {
        const size_t batch_size = options.batch_size ? options.batch_size : 1024;
        const auto t_start = std::chrono::steady_clock::now();
        last_ingest() = IngestStats();
        std::vector<std::unique_ptr<PinnedBuffer>> staged;   // the parsed columns: alive until the fence
        const csv::Text t = csv::load(path, options.has_headers, (char)options.delimiter.value_or((uint8_t)','), options.max_records);
        std::vector<size_t> sel;
        if (options.projection) {
            for (size_t i : *options.projection) {
                if (i >= t.header.size()) throw DataFrameError(DataFrameError::ComputeError, "csv projection index out of range");
                sel.push_back(i);
            }
        } else for (size_t i = 0; i < t.header.size(); ++i) sel.push_back(i);
        const size_t n = t.records.size();
        // The types of a long file are taken from its first records and every cell is parsed ONCE against them; a cell that does
        // not fit (or a column whose sampled cells were all empty) sends the file through inference over all records and a second
        // parse — the result is always what inference over the whole file gives.
        const size_t kSample = 16384;
        bool sampled = n > 4 * kSample;
        std::vector<csv::Inferred> types = csv::infer(t, sel, 0, sampled ? kSample : n);
        if (sampled) for (auto& ty : types) if (!ty.any) { sampled = false; break; }
        if (!sampled && n > 4 * kSample) types = csv::infer(t, sel);
        // typed values are parsed STRAIGHT into page-locked column buffers (+ bitmaps) by the worker threads, then every column
        // is queued for upload; one fence after the last one
        const int64_t bbytes = (int64_t)((n + 63) / 64 * 8 + 8);
        std::vector<uint8_t*> pvs, pbs;
        std::vector<int64_t> vbytes_of;
        auto buffers = [&]() {
            staged.clear();
            pvs.assign(sel.size(), nullptr); pbs.assign(sel.size(), nullptr); vbytes_of.assign(sel.size(), 0);
            for (size_t k = 0; k < sel.size(); ++k) {
                if (types[k].dtype == DataType::Utf8) continue;
                vbytes_of[k] = types[k].dtype == DataType::Boolean ? bbytes : (int64_t)(n * 8);
                staged.push_back(std::make_unique<PinnedBuffer>(vbytes_of[k] + bbytes));
                pvs[k] = staged.back()->data();
                pbs[k] = pvs[k] + vbytes_of[k];
                std::memset(pvs[k], 0, (size_t)(vbytes_of[k] + bbytes));
            }
        };
        buffers();
        std::vector<char> violated(sel.size(), 0);
        std::vector<csv::Filled> filled = csv::fill(t, sel, types, pvs, pbs, 0, sampled ? &violated : nullptr);
        if (sampled && std::find(violated.begin(), violated.end(), (char)1) != violated.end()) {
            types = csv::infer(t, sel);
            buffers();
            filled = csv::fill(t, sel, types, pvs, pbs);
        }
        for (size_t k = 0; k < sel.size(); ++k) types[k].any_null = filled[k].nulls > 0;
        std::vector<Column> cols;
        for (size_t k = 0; k < sel.size(); ++k) {
            const DataType dt = types[k].dtype;
            const bool any_null = types[k].any_null;
            std::vector<ArrayRef> chunks;
            if (dt == DataType::Utf8) {
                std::vector<std::string>& cells = filled[k].strings;
                for (size_t b = 0; b < n || chunks.empty(); b += batch_size) {
                    const size_t e = std::min(n, b + batch_size);
                    chunks.push_back(Array::from_strings(std::vector<std::string>(cells.begin() + b, cells.begin() + e)));
                    if (n == 0) break;
                }
            } else {
                const uint8_t* pv = pvs[k];
                const uint8_t* pb = pbs[k];
                const int64_t vbytes = vbytes_of[k];
                auto w = std::make_shared<Array>();
                w->dtype = dt;
                w->length = (int64_t)n;
                w->null_count = filled[k].nulls;
                w->values = std::make_shared<DeviceBuffer>(vbytes + 8);
                upload(w->values->data(), pv, dt == DataType::Boolean ? (int64_t)((n + 7) / 8) : vbytes, true);
                if (any_null) {
                    w->validity = std::make_shared<DeviceBuffer>(bbytes);
                    upload(w->validity->data(), pb, bbytes - 8, true);
                }
                ArrayRef whole = w;
                for (size_t b = 0; b < n || chunks.empty(); b += batch_size) {   // RecordBatches = zero-copy slices of the one buffer
                    auto c = std::const_pointer_cast<Array>(whole->slice((int64_t)b, (int64_t)std::min(batch_size, n - b)));
                    if (any_null) { c->null_count = 0; for (size_t r = b; r < std::min(n, b + batch_size); ++r) c->null_count += !((pb[r >> 3] >> (r & 7)) & 1); }
                    chunks.push_back(c);
                    if (n == 0) break;
                }
            }
            cols.push_back(Column::from_arrays(chunks, Field{t.header[sel[k]], dt, true}));
        }
        check(rdf_copy_fence());
        last_ingest().seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        return from_columns(std::move(cols));
    }

    // DataFrame::from_arrow (src/dataframe.rs:391-407: arrow::ipc::reader::FileReader -> Table::from_record_batches):
    // reads an Arrow IPC FILE or an IPC STREAM (told apart by the magic).  The flatbuffer metadata (Footer -> Schema,
    // Blocks; Message -> Schema / DictionaryBatch / RecordBatch) is decoded in place with a minimal reader; every column
    // buffer goes from the file image straight to HBM with one H2D copy (no per-value parsing, no intermediate arrays):
    // one chunk per record batch.  Primitive numeric and Boolean columns are on the compute path, Utf8 is carried
    // opaquely.  Dictionary-encoded columns (numeric or Utf8 values, any integer index type; delta and replacement
    // dictionaries of the stream format) are decoded while loading — the frame holds plain columns, as the reference's
    // kernels expect.  Nested types and compressed bodies are rejected with an error.
    // The file is read into ONE page-locked buffer; every record batch's column buffers are queued for upload straight out of
    // it (rdf_copy_h2d_async, the copy stream) while the next batch's metadata is decoded, and one fence ends the load:
    // no intermediate arrays, no runtime staging copy, no synchronisation per buffer.  last_ingest() tells what went up.
    static DataFrame from_arrow(const std::string& path) {
        const auto t0 = std::chrono::steady_clock::now();
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw DataFrameError(DataFrameError::IoError, "cannot open " + path);
        struct stat st;
        if (::fstat(fd, &st) != 0) { ::close(fd); throw DataFrameError(DataFrameError::IoError, "cannot stat " + path); }
        const size_t size = (size_t)st.st_size;
        // the file is MAPPED, not read into a page-locked copy: the metadata is decoded from the mapping and the column buffers
        // travel through the staging buffers of StagedUploader (page-locking 2.57 GB took 0.44 of the load's 0.49 s)
        void* map = size ? ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
        ::close(fd);
        if (size && map == MAP_FAILED) throw DataFrameError(DataFrameError::IoError, "cannot map " + path);
        last_ingest() = IngestStats();
        DataFrame df;
        try {
            IpcReader r((const uint8_t*)map, size);
            r.staged = true;
            if (size >= 20 && std::memcmp(map, "ARROW1", 6) == 0) r.read_file(); else r.read_stream();
            df = r.finish();
            StagedUploader::instance().finish();
        } catch (...) {
            try { StagedUploader::instance().finish(); } catch (...) {}
            if (map) ::munmap(map, size);
            throw;
        }
        if (map) ::munmap(map, size);
        last_ingest().seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return df;
    }
    // The same file as a HOST-resident frame: the file is mapped, its metadata decoded, and every primitive / Boolean column chunk
    // becomes a view into the mapping (nothing is uploaded, nothing is copied; the frame keeps the mapping alive).  What such a
    // frame is for: `LazyFrame::read(DataFrame::from_arrow_host(path)).filter(..).aggregate({}, ..).evaluate()` — Evaluate fuses
    // the steps into one rdf_pipeline call over RDF_MEM_HOST batches, which the library streams (slab k + 1 crosses the link while
    // the kernel runs over slab k): compute starts with the first slab instead of after the file is in HBM, and a file larger
    // than free HBM is aggregated in two slabs of it.  Utf8 columns ride along on the host as in from_arrow; dictionary-encoded
    // columns are refused (they are decoded on the device).  to_device() turns the frame into an ordinary device-resident one.
    static DataFrame from_arrow_host(const std::string& path) {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw DataFrameError(DataFrameError::IoError, "cannot open " + path);
        struct stat st;
        if (::fstat(fd, &st) != 0) { ::close(fd); throw DataFrameError(DataFrameError::IoError, "cannot stat " + path); }
        const size_t size = (size_t)st.st_size;
        void* map = size ? ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
        ::close(fd);
        if (size && map == MAP_FAILED) throw DataFrameError(DataFrameError::IoError, "cannot map " + path);
        if (!map) throw DataFrameError(DataFrameError::IoError, "Arrow IPC: empty file " + path);
        std::shared_ptr<void> keep(map, [size](void* p) { ::munmap(p, size); });
        IpcReader r((const uint8_t*)map, size);
        r.host_keep = keep;
        if (size >= 20 && std::memcmp(map, "ARROW1", 6) == 0) r.read_file(); else r.read_stream();
        return r.finish();
    }
    // every host-resident chunk uploaded (blocking copies; an already device-resident frame is returned as it is)
    DataFrame to_device() const {
        std::vector<Column> out;
        for (const Column& c : columns_) {
            std::vector<ArrayRef> arrs;
            for (const ArrayRef& a : c.data().chunks()) {
                if (!a->host) { arrs.push_back(a); continue; }
                auto d = std::make_shared<Array>(*a);
                d->host = false;
                const int64_t vb = a->dtype == DataType::Boolean ? (a->offset + a->length + 7) / 8 : (a->offset + a->length) * (int64_t)type_size(a->dtype);
                d->values = std::make_shared<DeviceBuffer>(vb + 8);
                if (vb > 0) check(rdf_copy_h2d(d->values->data(), a->values->data(), vb));
                if (a->validity) {
                    const int64_t bb = (a->offset + a->length + 7) / 8;
                    d->validity = std::make_shared<DeviceBuffer>(bb + 8);
                    if (bb > 0) check(rdf_copy_h2d(d->validity->data(), a->validity->data(), bb));
                }
                arrs.push_back(d);
            }
            out.push_back(Column::from_arrays(arrs, c.field()));
        }
        return from_columns(std::move(out));
    }
    // An image the caller holds: pinned in place (rdf_host_register) for the duration of the load when the platform allows it.
    static DataFrame from_arrow_image(const uint8_t* img, size_t size) {
        const auto t0 = std::chrono::steady_clock::now();
        last_ingest() = IngestStats();
        const bool reg = size > 0 && rdf_host_register(const_cast<uint8_t*>(img), (int64_t)size) == RDF_OK;
        DataFrame df;
        try { df = load_arrow_image(img, size, reg); }
        catch (...) { if (reg) { (void)rdf_copy_fence(); (void)rdf_host_unregister(const_cast<uint8_t*>(img)); } throw; }
        if (reg) check(rdf_host_unregister(const_cast<uint8_t*>(img)));
        last_ingest().seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return df;
    }
  private:
    static DataFrame load_arrow_image(const uint8_t* img, size_t size, bool pinned) {
        IpcReader r(img, size);
        r.pinned = pinned;
        try {
            if (size >= 20 && std::memcmp(img, "ARROW1", 6) == 0) r.read_file(); else r.read_stream();
            DataFrame df = r.finish();
            check(rdf_copy_fence());     // the image may go away (and kernels may run) after this
            return df;
        } catch (...) { (void)rdf_copy_fence(); throw; }
    }
  public:

  private:
    struct IpcReader {
        struct Dict { bool utf8 = false; DataType dt = DataType::Int64; std::vector<std::string> strs; std::vector<uint8_t> values; std::vector<bool> valid; int64_t n = 0; };
        struct Col { Field field; bool dict = false; int64_t dict_id = 0; DataType index_type = DataType::Int32; };
        const uint8_t* img; size_t size; FlatBuf fb;
        bool pinned = false;     // the image is page-locked: column buffers go up asynchronously, straight out of it
        bool staged = false;     // the image is pageable (a mapped file): column buffers go through StagedUploader
        std::shared_ptr<void> host_keep;   // set: nothing is uploaded — the arrays are views into the image, which this keeps alive
        std::vector<Col> cols;
        std::map<int64_t, Dict> dicts;
        std::vector<std::vector<ArrayRef>> chunks;
        IpcReader(const uint8_t* i, size_t n) : img(i), size(n), fb{i, n} {}
        static DataFrameError bad(const std::string& m) { return DataFrameError(DataFrameError::IoError, "Arrow IPC: " + m); }

        static DataType int_type(const FlatBuf& fb, size_t ty, const std::string& name) {   // Int { 0 bitWidth, 1 is_signed }
            const int bw = fb.scalar<int32_t>(ty, 0, 0);
            const bool sg = fb.scalar<uint8_t>(ty, 1, 0) != 0;
            switch (bw) {
                case 8: return sg ? DataType::Int8 : DataType::UInt8;
                case 16: return sg ? DataType::Int16 : DataType::UInt16;
                case 32: return sg ? DataType::Int32 : DataType::UInt32;
                case 64: return sg ? DataType::Int64 : DataType::UInt64;
                default: throw bad("integer width of column " + name);
            }
        }
        void read_schema(size_t schema_t) {   // Schema: 0 endianness, 1 fields
            if (!schema_t) throw bad("no schema");
            if (fb.scalar<int16_t>(schema_t, 0, 0) != 0) throw bad("big-endian data is not supported");
            const size_t fields_v = fb.field_pos(schema_t, 1);
            const size_t nfields = fb.vec_len(fields_v);
            for (size_t i = 0; i < nfields; ++i) {
                // Field: 0 name, 1 nullable, 2 type_type, 3 type, 4 dictionary, 5 children
                const size_t ft = fb.vec_table(fields_v, i);
                Col c;
                c.field.name = fb.string(ft, 0);
                c.field.nullable = fb.scalar<uint8_t>(ft, 1, 0) != 0;
                const int tt = fb.scalar<uint8_t>(ft, 2, 0);
                const size_t ty = fb.table_field(ft, 3);
                if (tt == 2) c.field.data_type = int_type(fb, ty, c.field.name);
                else if (tt == 3) {  // FloatingPoint { 0 precision: HALF, SINGLE, DOUBLE }
                    const int pr = fb.scalar<int16_t>(ty, 0, 0);
                    if (pr == 1) c.field.data_type = DataType::Float32; else if (pr == 2) c.field.data_type = DataType::Float64; else throw bad("half floats (column " + c.field.name + ")");
                } else if (tt == 6) c.field.data_type = DataType::Boolean;
                else if (tt == 5) c.field.data_type = DataType::Utf8;
                else throw bad("column " + c.field.name + ": unsupported type id " + std::to_string(tt));
                if (const size_t de = fb.table_field(ft, 4)) {   // DictionaryEncoding { 0 id, 1 indexType: Int (default int32), 2 isOrdered, 3 dictionaryKind }
                    c.dict = true;
                    c.dict_id = fb.scalar<int64_t>(de, 0, 0);
                    const size_t it = fb.table_field(de, 1);
                    c.index_type = it ? int_type(fb, it, c.field.name) : DataType::Int32;
                    if (c.field.data_type == DataType::Boolean) throw bad("dictionary of Boolean values (column " + c.field.name + ")");
                }
                cols.push_back(c);
            }
            chunks.assign(cols.size(), {});
        }
        struct Body { const uint8_t* p; int64_t len; };
        // one column's buffers out of a RecordBatch table: validity, values (Utf8: offsets, data)
        struct ColBufs { int64_t len, nulls, vo, vl, d0, dl, so, sl; };
        struct BatchCursor { size_t nodes_v, bufs_v, ni = 0, bi = 0; };
        ColBufs next_col(BatchCursor& cur, const Body& body, bool utf8) {
            if (cur.ni >= fb.vec_len(cur.nodes_v)) throw bad("field node list too short");
            const uint8_t* node = fb.vec_struct(cur.nodes_v, cur.ni++, 16);
            ColBufs b{};
            std::memcpy(&b.len, node, 8); std::memcpy(&b.nulls, node + 8, 8);
            auto next_buf = [&](int64_t& bo, int64_t& bl) {
                if (cur.bi >= fb.vec_len(cur.bufs_v)) throw bad("buffer list too short");
                const uint8_t* p = fb.vec_struct(cur.bufs_v, cur.bi++, 16);
                std::memcpy(&bo, p, 8); std::memcpy(&bl, p + 8, 8);
                if (bo < 0 || bl < 0 || bo + bl > body.len) throw bad("buffer out of bounds");
            };
            next_buf(b.vo, b.vl);
            next_buf(b.d0, b.dl);
            if (utf8) next_buf(b.so, b.sl);
            if (b.len < 0 || (b.nulls > 0 && b.vl < (b.len + 7) / 8)) throw bad("validity buffer too short");
            return b;
        }
        static bool bit(const uint8_t* p, int64_t i) { return (p[i >> 3] >> (i & 7)) & 1; }
        std::vector<std::string> read_strings(const ColBufs& b, const Body& body) {
            if (b.dl < 4 * (b.len + 1) && b.len > 0) throw bad("string offsets buffer too short");
            std::vector<std::string> strs((size_t)b.len);
            for (int64_t r = 0; r < b.len; ++r) {
                int32_t a0, a1;
                std::memcpy(&a0, body.p + b.d0 + 4 * r, 4); std::memcpy(&a1, body.p + b.d0 + 4 * (r + 1), 4);
                if (a0 < 0 || a1 < a0 || a1 > b.sl) throw bad("string offsets out of bounds");
                strs[(size_t)r].assign((const char*)body.p + b.so + a0, (size_t)(a1 - a0));
            }
            return strs;
        }
        static ArrayRef strings_with_validity(std::vector<std::string> strs, const std::vector<bool>* valid) {
            auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(strs)));
            if (valid) {
                const auto bits = pack_bits(*valid);
                a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size() + 8);
                check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
                for (bool v : *valid) a->null_count += !v;
            }
            return a;
        }
        // RecordBatch: 0 length, 1 nodes [FieldNode{int64 length, int64 null_count}], 2 buffers [Buffer{int64 offset, int64 length}], 3 compression
        void read_record_batch(size_t rb, const Body& body) {
            if (fb.field_pos(rb, 3)) throw bad("compressed record batches are not supported");
            const int64_t nrows = fb.scalar<int64_t>(rb, 0, 0);
            BatchCursor cur{fb.field_pos(rb, 1), fb.field_pos(rb, 2)};
            if (fb.vec_len(cur.nodes_v) != cols.size()) throw bad("nested columns are not supported");
            for (size_t c = 0; c < cols.size(); ++c) {
                const Col& col = cols[c];
                const DataType dt = col.field.data_type;
                const ColBufs b = next_col(cur, body, dt == DataType::Utf8 && !col.dict);
                if (b.len != nrows) throw bad("column length differs from the batch length");
                if (col.dict && host_keep) throw bad("dictionary-encoded column " + col.field.name + " is decoded on the device: load the file with from_arrow()");
                if (col.dict) { chunks[c].push_back(decode_dictionary_column(col, b, body)); continue; }
                if (dt == DataType::Utf8) {
                    std::vector<bool> valid;
                    if (b.nulls > 0) { valid.resize((size_t)b.len); for (int64_t r = 0; r < b.len; ++r) valid[(size_t)r] = bit(body.p + b.vo, r); }
                    chunks[c].push_back(strings_with_validity(read_strings(b, body), b.nulls > 0 ? &valid : nullptr));
                    continue;
                }
                const int64_t need = dt == DataType::Boolean ? (b.len + 7) / 8 : b.len * (int64_t)type_size(dt);
                if (b.dl < need) throw bad("values buffer of column " + col.field.name + " is too short");
                auto a = std::make_shared<Array>();
                a->dtype = dt;
                a->length = b.len;
                if (host_keep) {     // a view: the values and the bitmap stay where the file's image has them
                    a->host = true;
                    a->values = std::make_shared<DeviceBuffer>(const_cast<uint8_t*>(body.p + b.d0), need, host_keep);
                    if (b.nulls > 0) {
                        a->validity = std::make_shared<DeviceBuffer>(const_cast<uint8_t*>(body.p + b.vo), (b.len + 7) / 8, host_keep);
                        a->null_count = b.nulls;
                    }
                    chunks[c].push_back(a);
                    continue;
                }
                a->values = std::make_shared<DeviceBuffer>(need + 8);
                if (staged) StagedUploader::instance().push(a->values->data(), body.p + b.d0, need); else upload(a->values->data(), body.p + b.d0, need, pinned);
                if (b.nulls > 0) {
                    a->validity = std::make_shared<DeviceBuffer>((b.len + 7) / 8 + 8);
                    if (staged) StagedUploader::instance().push(a->validity->data(), body.p + b.vo, (b.len + 7) / 8); else upload(a->validity->data(), body.p + b.vo, (b.len + 7) / 8, pinned);
                    a->null_count = b.nulls;
                }
                chunks[c].push_back(a);
            }
        }
        // DictionaryBatch { 0 id, 1 data: RecordBatch (one column = the dictionary's values), 2 isDelta }
        void read_dictionary_batch(size_t db, const Body& body) {
            const int64_t id = fb.scalar<int64_t>(db, 0, 0);
            const bool delta = fb.scalar<uint8_t>(db, 2, 0) != 0;
            const size_t rb = fb.table_field(db, 1);
            if (!rb) throw bad("dictionary batch without data");
            if (fb.field_pos(rb, 3)) throw bad("compressed dictionary batches are not supported");
            const Col* owner = nullptr;
            for (auto& c : cols) if (c.dict && c.dict_id == id) owner = &c;
            if (!owner) throw bad("dictionary " + std::to_string(id) + " belongs to no column");
            BatchCursor cur{fb.field_pos(rb, 1), fb.field_pos(rb, 2)};
            const bool utf8 = owner->field.data_type == DataType::Utf8;
            const ColBufs b = next_col(cur, body, utf8);
            Dict fresh;
            Dict& d = delta && dicts.count(id) ? dicts[id] : fresh;
            d.utf8 = utf8; d.dt = owner->field.data_type;
            for (int64_t r = 0; r < b.len; ++r) d.valid.push_back(b.nulls > 0 ? bit(body.p + b.vo, r) : true);
            if (utf8) { auto s = read_strings(b, body); d.strs.insert(d.strs.end(), s.begin(), s.end()); }
            else {
                const int64_t es = (int64_t)type_size(d.dt);
                if (b.dl < b.len * es) throw bad("dictionary values buffer too short");
                d.values.insert(d.values.end(), body.p + b.d0, body.p + b.d0 + b.len * es);
            }
            d.n += b.len;
            if (&d == &fresh) dicts[id] = std::move(fresh);   // first sight of the id, or a replacement dictionary (stream format)
        }
        ArrayRef decode_dictionary_column(const Col& col, const ColBufs& b, const Body& body) {
            auto it = dicts.find(col.dict_id);
            if (it == dicts.end()) throw bad("record batch before the dictionary of column " + col.field.name);
            const Dict& d = it->second;
            const int64_t is = (int64_t)type_size(col.index_type);
            if (b.dl < b.len * is) throw bad("index buffer of column " + col.field.name + " is too short");
            const bool sg = col.index_type == DataType::Int8 || col.index_type == DataType::Int16 || col.index_type == DataType::Int32 || col.index_type == DataType::Int64;
            std::vector<bool> valid((size_t)b.len, true);
            bool any_null = false;
            std::vector<int64_t> idx((size_t)b.len, 0);
            for (int64_t r = 0; r < b.len; ++r) {
                if (b.nulls > 0 && !bit(body.p + b.vo, r)) { valid[(size_t)r] = false; any_null = true; continue; }
                uint64_t raw = 0;
                std::memcpy(&raw, body.p + b.d0 + r * is, (size_t)is);
                int64_t v = (int64_t)raw;
                if (sg && is < 8) { const int sh = 64 - 8 * (int)is; v = (int64_t)(raw << sh) >> sh; }
                if (v < 0 || v >= d.n) throw bad("dictionary index out of range in column " + col.field.name);
                if (!d.valid[(size_t)v]) { valid[(size_t)r] = false; any_null = true; continue; }
                idx[(size_t)r] = v;
            }
            if (d.utf8) {
                std::vector<std::string> strs((size_t)b.len);
                for (int64_t r = 0; r < b.len; ++r) if (valid[(size_t)r]) strs[(size_t)r] = d.strs[(size_t)idx[(size_t)r]];
                return strings_with_validity(std::move(strs), any_null ? &valid : nullptr);
            }
            const int64_t es = (int64_t)type_size(d.dt);
            std::vector<uint8_t> vals((size_t)(b.len * es) + 8, 0);
            for (int64_t r = 0; r < b.len; ++r) if (valid[(size_t)r]) std::memcpy(vals.data() + r * es, d.values.data() + idx[(size_t)r] * es, (size_t)es);
            auto a = std::make_shared<Array>();
            a->dtype = d.dt;
            a->length = b.len;
            a->values = std::make_shared<DeviceBuffer>(b.len * es + 8);
            if (b.len) check(rdf_copy_h2d(a->values->data(), vals.data(), b.len * es));
            if (any_null) {
                const auto bits = pack_bits(valid);
                a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size() + 8);
                check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
                for (bool v : valid) a->null_count += !v;
            }
            return a;
        }
        // one encapsulated message at `pos`: [0xFFFFFFFF] int32 metadata length, flatbuffer Message, body.  Returns the position
        // behind the body, 0 at the end-of-stream marker.  Message: 0 version, 1 header_type, 2 header, 3 bodyLength
        size_t read_message(size_t pos, int64_t known_body_len, bool want_batches_only) {
            if (pos + 4 > size) return 0;
            uint32_t first;
            std::memcpy(&first, img + pos, 4);
            size_t mpos = pos + 4;
            uint32_t meta_len = first;
            if (first == 0xFFFFFFFFu) { if (pos + 8 > size) return 0; std::memcpy(&meta_len, img + pos + 4, 4); mpos = pos + 8; }
            if (meta_len == 0) return 0;   // end of stream
            if (mpos + meta_len > size) throw bad("message metadata out of bounds");
            const size_t msg = fb.root(mpos);
            const int kind = fb.scalar<uint8_t>(msg, 1, 0);
            const int64_t body_len = known_body_len >= 0 ? known_body_len : fb.scalar<int64_t>(msg, 3, 0);
            const size_t body_pos = mpos + meta_len;
            if (body_len < 0 || body_pos + (uint64_t)body_len > size) throw bad("message body out of bounds");
            const Body body{img + body_pos, body_len};
            const size_t hdr = fb.table_field(msg, 2);
            if (kind == 1) { if (!want_batches_only && cols.empty()) read_schema(hdr); }
            else if (kind == 2) read_dictionary_batch(hdr, body);
            else if (kind == 3) read_record_batch(hdr, body);
            else throw bad("unsupported message type " + std::to_string(kind));
            return body_pos + (size_t)body_len;
        }
        void read_stream() {
            size_t pos = 0;
            while (pos < size) {
                const size_t next = read_message(pos, -1, false);
                if (!next) break;
                if (cols.empty()) throw bad("stream does not start with a schema");
                pos = (next + 7) & ~(size_t)7;
            }
            if (cols.empty()) throw bad("not an Arrow IPC file or stream");
        }
        void read_file() {
            if (std::memcmp(img + size - 6, "ARROW1", 6) != 0) throw bad("not an Arrow IPC file (magic)");
            int32_t flen;
            std::memcpy(&flen, img + size - 10, 4);
            if (flen <= 0 || (size_t)flen + 18 > size) throw bad("bad footer length");
            const size_t footer = fb.root(size - 10 - (size_t)flen);
            // Footer: 0 version, 1 schema, 2 dictionaries, 3 recordBatches; Block { int64 offset; int32 metaDataLength; (pad) int64 bodyLength } = 24 bytes
            read_schema(fb.table_field(footer, 1));
            for (int list : {2, 3}) {
                const size_t blocks_v = fb.field_pos(footer, list);
                for (size_t b = 0; b < fb.vec_len(blocks_v); ++b) {
                    const uint8_t* blk = fb.vec_struct(blocks_v, b, 24);
                    int64_t off, body_len; int32_t meta_len;
                    std::memcpy(&off, blk, 8); std::memcpy(&meta_len, blk + 8, 4); std::memcpy(&body_len, blk + 16, 8);
                    if (off < 0 || meta_len < 8 || body_len < 0 || (uint64_t)off + (uint64_t)meta_len + (uint64_t)body_len > size) throw bad("block out of bounds");
                    read_message((size_t)off, body_len, true);
                }
            }
        }
        DataFrame finish() {
            std::vector<Column> out;
            for (size_t c = 0; c < cols.size(); ++c) {
                if (chunks[c].empty()) {   // no record batches: the schema alone, one empty chunk per column
                    if (cols[c].field.data_type == DataType::Utf8) chunks[c].push_back(Array::from_strings({}));
                    else chunks[c].push_back(Array::make_out(cols[c].field.data_type, 0, false));
                }
                out.push_back(Column::from_arrays(chunks[c], cols[c].field));
            }
            return from_columns(std::move(out));
        }
    };

  public:
    const Schema& schema() const { return schema_; }
    size_t num_columns() const { return columns_.size(); }
    size_t num_chunks() const { return columns_.empty() ? 0 : columns_[0].data().num_chunks(); }
    int64_t num_rows() const { return columns_.empty() ? 0 : columns_[0].num_rows(); }
    const Column& column(size_t i) const { return columns_[i]; }
    const std::vector<Column>& columns() const { return columns_; }
    const Column& column_by_name(const std::string& name) const {
        auto c = schema_.column_with_name(name);
        if (!c) throw DataFrameError(DataFrameError::ComputeError, "Column not found by name: " + name);
        return columns_[c->first];
    }
    bool has_column(const std::string& name) const { return schema_.column_with_name(name).has_value(); }

    // :97-113 — an existing column of that name is dropped, the new one goes last
    DataFrame with_column(const std::string& name, Column column) const {
        DataFrame d = has_column(name) ? drop({name}) : *this;
        column = column.renamed(name);
        d.schema_.fields.push_back(column.field());
        d.columns_.push_back(std::move(column));
        return d;
    }
    DataFrame with_column_renamed(const std::string& old_name, const std::string& new_name) const {  // :116-124
        DataFrame d = *this;
        auto c = schema_.column_with_name(old_name);
        if (!c) throw DataFrameError(DataFrameError::NoneError, "column " + old_name + " not found");
        d.schema_.fields[c->first].name = new_name;
        d.columns_[c->first] = d.columns_[c->first].renamed(new_name);
        return d;
    }
    // :128-163 — chunk i of every column = RecordBatch i
    std::vector<RecordBatch> to_record_batches() const {
        std::vector<RecordBatch> out;
        for (size_t i = 0; i < num_chunks(); ++i) {
            RecordBatch b;
            b.schema = schema_;
            for (auto& c : columns_) b.columns.push_back(c.data().chunk(i));
            out.push_back(std::move(b));
        }
        return out;
    }
    // DataFrame::with_id (:234-249): a UInt64 column counting from 100 000 * chunk index + 1 within every chunk (the
    // reference's "no record batch has 100k rows" assumption included).  The ids are built on the host and uploaded.
    DataFrame with_id(const std::string& name) const {
        std::vector<ArrayRef> arrays;
        if (!columns_.empty()) {
            size_t index = 0;
            for (auto& ch : columns_[0].data().chunks()) {
                std::vector<uint64_t> ids((size_t)ch->length);
                for (size_t i = 0; i < ids.size(); ++i) ids[i] = 100000ull * index + 1 + i;
                arrays.push_back(Array::from_vec<uint64_t>(ids));
                ++index;
            }
        }
        return with_column(name, Column::from_arrays(arrays, Field{name, DataType::UInt64, false}));
    }
    DataFrame limit(size_t count) const {  // :166-175, zero-copy slices
        std::vector<Column> cols;
        for (auto& c : columns_) cols.push_back(c.slice(0, (int64_t)count));
        return DataFrame(schema_, std::move(cols));
    }
    DataFrame select(const std::vector<std::string>& names) const {  // :258-297 — unknown names are omitted; "*" keeps every column (:272)
        for (auto& n : names) if (n == "*") return *this;
        Schema s; std::vector<Column> cols;
        for (size_t i = 0; i < columns_.size(); ++i)
            for (auto& n : names) if (schema_.fields[i].name == n) { s.fields.push_back(schema_.fields[i]); cols.push_back(columns_[i]); break; }
        return DataFrame(std::move(s), std::move(cols));
    }
    DataFrame drop(const std::vector<std::string>& names) const {  // :302-337
        Schema s; std::vector<Column> cols;
        for (size_t i = 0; i < columns_.size(); ++i) {
            bool dropped = false;
            for (auto& n : names) dropped |= schema_.fields[i].name == n;
            if (!dropped) { s.fields.push_back(schema_.fields[i]); cols.push_back(columns_[i]); }
        }
        return DataFrame(std::move(s), std::move(cols));
    }

    // evaluate_boolean_filter (:612-624): one BooleanArray mask per RecordBatch, computed in ONE launch
    Column evaluate_boolean_filter(const FilterRef& filter) const {
        // The text leaves — a comparison or starts_with / ends_with / contains / like / rlike over a Utf8 column and a String scalar,
        // or a comparison of two Utf8 columns — are evaluated on their own (rdf_utf8_predicate / rdf_utf8_compare) into Boolean
        // columns that stand in for them, under private names, in what rdf_predicate then evaluates.
        std::vector<std::pair<std::string, Column>> leaves;
        const FilterRef rest = lower_text_leaves(filter, leaves);
        if (!leaves.empty()) {
            if (rest->kind == BooleanFilter::InputColumn) return leaves[0].second;   // the tree was one text leaf
            DataFrame with = *this;
            for (auto& l : leaves) with = with.with_column(l.first, l.second);
            return with.evaluate_boolean_filter(rest);
        }
        Lowered low;
        const int root = low.add(filter_to_expr(filter, [this](const std::string& n) {
            if (!has_column(n)) throw DataFrameError(DataFrameError::ComputeError, "Cannot find column " + n);  // expression.rs:812-815
            return Expr::col(n);
        }));
        return run_predicate(low, root);
    }
    bool is_text_column(const FilterRef& f) const {
        return f && f->kind == BooleanFilter::InputColumn && has_column(f->column_name) && column_by_name(f->column_name).data_type() == DataType::Utf8;
    }
    static bool is_text_scalar(const FilterRef& f) { return f && f->kind == BooleanFilter::InputScalar && f->scalar_v.kind == Scalar::String; }
    FilterRef lower_text_leaves(const FilterRef& f, std::vector<std::pair<std::string, Column>>& leaves) const {
        if (!f) return f;
        if (f->kind == BooleanFilter::IsIn) {   // a membership leaf: its mask stands in for it like a text leaf's
            if (!f->l || f->l->kind != BooleanFilter::InputColumn || !f->set_v) throw DataFrameError(DataFrameError::ComputeError, "is_in takes a column and a column of values");
            const std::string name = std::string("\x01is_in_") + std::to_string(leaves.size());
            leaves.emplace_back(name, member_mask(DataFrame::from_columns({*f->set_v}), {{f->l->column_name, f->set_v->name()}}, RDF_MEMBER_IS_IN, name));
            return BooleanFilter::column(name);
        }
        int32_t op = -1;
        bool comparison = true;
        switch (f->kind) {
            case BooleanFilter::Eq: op = RDF_UTF8_EQ; break;
            case BooleanFilter::Ne: op = RDF_UTF8_NE; break;
            case BooleanFilter::Lt: op = RDF_UTF8_LT; break;
            case BooleanFilter::Le: op = RDF_UTF8_LE; break;
            case BooleanFilter::Gt: op = RDF_UTF8_GT; break;
            case BooleanFilter::Ge: op = RDF_UTF8_GE; break;
            case BooleanFilter::StartsWith: op = RDF_UTF8_STARTS_WITH; comparison = false; break;
            case BooleanFilter::EndsWith: op = RDF_UTF8_ENDS_WITH; comparison = false; break;
            case BooleanFilter::Contains: op = RDF_UTF8_CONTAINS; comparison = false; break;
            case BooleanFilter::Like: op = RDF_UTF8_LIKE; comparison = false; break;
            case BooleanFilter::RLike: comparison = false; break;   // op stays -1: rdf_utf8_regexp_match, not rdf_utf8_predicate
            case BooleanFilter::Not: case BooleanFilter::And: case BooleanFilter::Or: {
                auto g = std::make_shared<BooleanFilter>(*f);
                g->l = lower_text_leaves(f->l, leaves);
                g->r = lower_text_leaves(f->r, leaves);
                return g;
            }
            default: return f;
        }
        const bool on_host = is_host();
        Column mask;
        if (f->kind == BooleanFilter::RLike) {
            if (!is_text_column(f->l) || !is_text_scalar(f->r)) return f;
            mask = column_by_name(f->l->column_name).rlike(f->r->scalar_v.s, on_host);
        } else if (is_text_column(f->l) && is_text_scalar(f->r)) {
            mask = column_by_name(f->l->column_name).utf8_predicate(op, f->r->scalar_v.s, f->escape, on_host);
        } else if (comparison && is_text_scalar(f->l) && is_text_column(f->r)) {   // 'x' < col  is  col > 'x'
            static const int32_t flipped[6] = {RDF_UTF8_EQ, RDF_UTF8_NE, RDF_UTF8_GT, RDF_UTF8_GE, RDF_UTF8_LT, RDF_UTF8_LE};
            mask = column_by_name(f->r->column_name).utf8_predicate(flipped[op], f->l->scalar_v.s, -1, on_host);
        } else if (comparison && is_text_column(f->l) && is_text_column(f->r)) {
            mask = column_by_name(f->l->column_name).utf8_compare(op, column_by_name(f->r->column_name), on_host);
        } else {
            return f;   // not a text leaf: the numeric path takes it, or refuses it
        }
        const std::string name = std::string("\x01utf8_pred_") + std::to_string(leaves.size());
        leaves.emplace_back(name, mask);
        return BooleanFilter::column(name);
    }
    Column run_predicate(const Lowered& low, int root) const {
        const size_t nch = num_chunks();
        std::vector<rdf_array> cols;
        bool nullable = false;
        for (auto& n : low.columns)
            for (auto& a : column_by_name(n).data().chunks()) { cols.push_back(a->view()); nullable |= a->validity != nullptr; }
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        const auto counts = columns_[0].data().chunk_counts();
        const bool on_host = is_host();
        for (size_t i = 0; i < nch; ++i) { outs.push_back(Array::make_out(DataType::Boolean, counts[i], nullable, on_host)); ov.push_back(outs.back()->out_view(counts[i])); }
        if (low.columns.empty()) {  // constant predicate: the batch length comes from column 0
            for (auto& a : columns_[0].data().chunks()) cols.push_back(a->view());
            check(rdf_predicate(low.nodes.data(), (int32_t)low.nodes.size(), root, cols.data(), 1, (int64_t)nch, ov.data()));
        } else
            check(rdf_predicate(low.nodes.data(), (int32_t)low.nodes.size(), root, cols.data(), (int32_t)low.columns.size(), (int64_t)nch, ov.data()));
        std::vector<ArrayRef> res;
        for (size_t i = 0; i < nch; ++i) { outs[i]->length = ov[i].length; outs[i]->null_count = ov[i].null_count; res.push_back(outs[i]); }
        return Column::from_arrays(res, Field{"bool_filter", DataType::Boolean, true});
    }
    // the frame's numeric / Boolean column chunks are views into host memory (from_arrow_host, or the result of an operator over such a frame)
    bool is_host() const {
        for (auto& c : columns_) for (auto& a : c.data().chunks()) if (a->dtype != DataType::Utf8 && a->host) return true;
        return false;
    }
    // ... ALL of them are (a host frame with a device-computed column added is not: the streamed calls take host chunks only)
    bool all_host() const {
        bool any = false;
        for (auto& c : columns_) for (auto& a : c.data().chunks()) if (a->dtype != DataType::Utf8) { if (!a->host) return false; any = true; }
        return any;
    }
    // DataFrame::filter (:178-189): the mask, then EVERY column compacted by it in one pass (rdf_filter_columns).
    // A host-resident frame of numeric columns takes ONE call instead (rdf_filter_pipeline): predicate and compaction run on the
    // device slab by slab while the next slab comes in and the kept rows of the previous one go back — the result is a
    // host-resident frame again, and a frame larger than free HBM is filtered all the same.
    DataFrame filter(const FilterRef& condition) const {
        bool all_numeric = !columns_.empty();
        for (auto& c : columns_) all_numeric = all_numeric && (is_integer(c.data_type()) || is_float(c.data_type()));
        if (!(all_host() && all_numeric && columns_.size() <= 64) || has_is_in(condition)) return filter_by_mask(evaluate_boolean_filter(condition));
        Lowered low;
        const int root = low.add(filter_to_expr(condition, [this](const std::string& n) {
            if (!has_column(n)) throw DataFrameError(DataFrameError::ComputeError, "Cannot find column " + n);
            return Expr::col(n);
        }));
        // the call's column order: the predicate's columns first (the expression indexes them), then the rest of the frame
        std::vector<size_t> order;
        for (auto& n : low.columns) order.push_back(schema_.column_with_name(n)->first);
        for (size_t k = 0; k < columns_.size(); ++k) if (std::find(order.begin(), order.end(), k) == order.end()) order.push_back(k);
        if (order.size() != columns_.size()) return filter_by_mask(evaluate_boolean_filter(condition));   // (a column named twice by the predicate's lowering)
        const size_t nch = num_chunks();
        std::vector<rdf_array> cv;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t k : order)
            for (auto& a : columns_[k].data().chunks()) {
                cv.push_back(a->view());
                outs.push_back(Array::make_out(a->dtype, a->length, a->validity != nullptr, true));
                ov.push_back(outs.back()->out_view(a->length));
            }
        check(rdf_filter_pipeline(low.nodes.data(), (int32_t)low.nodes.size(), root, cv.data(), (int32_t)order.size(), (int64_t)nch, ov.data()));
        std::vector<Column> result(columns_.size());
        for (size_t j = 0; j < order.size(); ++j) {
            std::vector<ArrayRef> chunks;
            for (size_t i = 0; i < nch; ++i) {
                auto& o = outs[j * nch + i];
                o->length = ov[j * nch + i].length;
                o->null_count = ov[j * nch + i].null_count;
                chunks.push_back(o);
            }
            result[order[j]] = Column::from_arrays(chunks, columns_[order[j]].field());
        }
        return DataFrame(schema_, std::move(result));
    }
    static bool has_is_in(const FilterRef& f) { return f && (f->kind == BooleanFilter::IsIn || has_is_in(f->l) || has_is_in(f->r)); }
    DataFrame filter_by_mask(const Column& mask) const {
        const size_t nch = num_chunks();
        const auto mv = mask.data().views();
        std::vector<int64_t> counts(nch);
        check(rdf_filter_count(mv.data(), (int64_t)nch, counts.data()));
        std::vector<Column> result(columns_.size());
        for (size_t base = 0; base < columns_.size(); base += 256) {  // rdf_filter_columns takes up to 256 columns per call
            const size_t n = std::min<size_t>(256, columns_.size() - base);
            std::vector<rdf_array> cv;
            std::vector<std::shared_ptr<Array>> outs;
            std::vector<rdf_out> ov;
            std::vector<std::vector<ArrayRef>> widened(n);   // Boolean columns travel through the compaction as UInt8 (cast there and back on the device)
            for (size_t k = 0; k < n; ++k) {
                const Column& c = columns_[base + k];
                const bool is_bool = c.data_type() == DataType::Boolean;
                if (is_bool) widened[k] = cast_arrays(c.data().chunks(), DataType::UInt8);
                for (size_t i = 0; i < nch; ++i) {
                    const ArrayRef& src = is_bool ? widened[k][i] : c.data().chunk(i);
                    if (c.data_type() == DataType::Utf8) {   // opaque host strings: a placeholder keeps the column count of the call
                        cv.push_back(rdf_array{}); outs.push_back(nullptr); ov.push_back(rdf_out{});
                        continue;
                    }
                    cv.push_back(src->view());
                    outs.push_back(Array::make_out(is_bool ? DataType::UInt8 : c.data_type(), counts[i], src->validity != nullptr, src->host));
                    ov.push_back(outs.back()->out_view(counts[i]));
                }
            }
            // device columns of this group, packed without the Utf8 placeholders
            std::vector<rdf_array> dcv; std::vector<rdf_out> dov; std::vector<size_t> dmap;
            for (size_t k = 0; k < n; ++k)
                if (columns_[base + k].data_type() != DataType::Utf8) { dmap.push_back(k); for (size_t i = 0; i < nch; ++i) { dcv.push_back(cv[k * nch + i]); dov.push_back(ov[k * nch + i]); } }
            if (!dmap.empty()) check(rdf_filter_columns(dcv.data(), (int32_t)dmap.size(), mv.data(), (int64_t)nch, dov.data()));
            for (size_t d = 0; d < dmap.size(); ++d) {
                const size_t k = dmap[d];
                std::vector<ArrayRef> chunks;
                for (size_t i = 0; i < nch; ++i) { auto& o = outs[k * nch + i]; o->length = dov[d * nch + i].length; o->null_count = dov[d * nch + i].null_count; chunks.push_back(o); }
                if (columns_[base + k].data_type() == DataType::Boolean) chunks = cast_arrays(chunks, DataType::Boolean);
                result[base + k] = Column::from_arrays(chunks, columns_[base + k].field());
            }
        }
        // Utf8 columns are carried on the host: filtered there with the mask's bits (value AND validity, like Column::filter)
        bool any_text = false;
        for (auto& c : columns_) any_text |= c.data_type() == DataType::Utf8;
        if (any_text) {
            std::vector<std::vector<bool>> keep(nch);
            for (size_t i = 0; i < nch; ++i) {
                const auto bits = mask.data().chunk(i)->bools_to_host(), valid = mask.data().chunk(i)->valid_to_host();
                keep[i].resize(bits.size());
                for (size_t r = 0; r < bits.size(); ++r) keep[i][r] = bits[r] && valid[r];
            }
            for (size_t k = 0; k < columns_.size(); ++k) {
                if (columns_[k].data_type() != DataType::Utf8) continue;
                std::vector<ArrayRef> chunks;
                for (size_t i = 0; i < nch; ++i) {
                    const auto& src = *columns_[k].data().chunk(i)->strings;
                    std::vector<std::string> out;
                    const size_t first = (size_t)columns_[k].data().chunk(i)->offset;
                    for (size_t r = 0; r < keep[i].size(); ++r) if (keep[i][r]) out.push_back(src[first + r]);
                    chunks.push_back(Array::from_strings(std::move(out)));
                }
                result[k] = Column::from_arrays(chunks, columns_[k].field());
            }
        }
        return DataFrame(schema_, std::move(result));
    }
    // DataFrame::join (:626-719): equi-join indices on 1..4 key column pairs, then Column::take of every column
    // of both frames (left columns first).  JoinType as src/expression.rs:339-345.
    // LeftSemi / LeftAnti (values beyond rdf_join_type: rdf_equijoin_indices* never sees them) keep the LEFT frame's columns only:
    // the rows with / without a partner, through rdf_member_mask and the frame filter.
    enum class JoinType { LeftJoin = RDF_JOIN_LEFT, RightJoin = RDF_JOIN_RIGHT, InnerJoin = RDF_JOIN_INNER, FullJoin = RDF_JOIN_FULL,
                          LeftSemi = 100, LeftAnti = 101 };
    struct JoinCriteria { JoinType join_type; std::vector<std::pair<std::string, std::string>> criteria; };
    DataFrame join(const DataFrame& other, const JoinCriteria& jc) const {
        if (jc.criteria.empty() || jc.criteria.size() > 4) throw DataFrameError(DataFrameError::ComputeError, "join: 1 to 4 key column pairs");
        if (jc.join_type == JoinType::LeftSemi || jc.join_type == JoinType::LeftAnti)
            return filter_by_mask(member_mask(other, jc.criteria, jc.join_type == JoinType::LeftSemi ? RDF_MEMBER_SEMI : RDF_MEMBER_ANTI, "\x01member"));
        // key pair k: this[criteria[k].first] against other[criteria[k].second], laid out [k * nchunks + chunk]
        std::vector<rdf_array> lk, rk;
        for (auto& c : jc.criteria) {
            if (column_by_name(c.first).data_type() == DataType::Utf8 || other.column_by_name(c.second).data_type() == DataType::Utf8) continue;
            for (auto& v : column_by_name(c.first).data().views()) lk.push_back(v);
            for (auto& v : other.column_by_name(c.second).data().views()) rk.push_back(v);
        }
        const int32_t nk = (int32_t)jc.criteria.size();
        const int64_t lnc = (int64_t)num_chunks(), rnc = (int64_t)other.num_chunks();
        int64_t rows = 0;
        bool any_text = false;
        for (auto& c : jc.criteria) any_text |= column_by_name(c.first).data_type() == DataType::Utf8 || other.column_by_name(c.second).data_type() == DataType::Utf8;
        if (any_text) {   // a text pair is dictionary-encoded against one dictionary of both sides (rdf_equijoin_indices_keys)
            for (auto& c : jc.criteria)
                if ((column_by_name(c.first).data_type() == DataType::Utf8) != (other.column_by_name(c.second).data_type() == DataType::Utf8))
                    throw DataFrameError(DataFrameError::ComputeError, "Join columns must have compatible types");
            const bool host = numeric_columns_on_host() && other.numeric_columns_on_host();
            std::vector<SortCriteria> lc, rc;
            for (auto& c : jc.criteria) { lc.push_back(SortCriteria{c.first, false, false}); rc.push_back(SortCriteria{c.second, false, false}); }
            const SortKeys lsk = sort_keys(lc, host), rsk = other.sort_keys(rc, host);
            check(rdf_equijoin_indices_keys(lsk.keys.data(), lnc, rsk.keys.data(), rnc, nk, (int32_t)jc.join_type, nullptr, nullptr, &rows));
            auto li = Array::make_out(DataType::UInt32, rows, true, host), ri = Array::make_out(DataType::UInt32, rows, true, host);
            rdf_out lo = li->out_view(rows), ro = ri->out_view(rows);
            check(rdf_equijoin_indices_keys(lsk.keys.data(), lnc, rsk.keys.data(), rnc, nk, (int32_t)jc.join_type, &lo, &ro, &rows));
            li->length = ri->length = rows;
            li->null_count = lo.null_count; ri->null_count = ro.null_count;
            std::vector<Column> cols;
            for (auto& c : columns_) cols.push_back(c.take(li, 4096));
            for (auto& c : other.columns_) cols.push_back(c.take(ri, 4096));
            return DataFrame::from_columns(cols);
        }
        check(rdf_equijoin_indices_multi(lk.data(), lnc, rk.data(), rnc, nk, (int32_t)jc.join_type, nullptr, nullptr, &rows));
        auto li = Array::make_out(DataType::UInt32, rows, true), ri = Array::make_out(DataType::UInt32, rows, true);
        rdf_out lo = li->out_view(rows), ro = ri->out_view(rows);
        check(rdf_equijoin_indices_multi(lk.data(), lnc, rk.data(), rnc, nk, (int32_t)jc.join_type, &lo, &ro, &rows));
        li->length = ri->length = rows;
        li->null_count = lo.null_count; ri->null_count = ro.null_count;
        std::vector<Column> cols;
        for (auto& c : columns_) cols.push_back(c.take(li, 4096));
        for (auto& c : other.columns_) cols.push_back(c.take(ri, 4096));
        return DataFrame::from_columns(cols);
    }
    // DataFrame::sort (:194-214): lexsort_to_indices over the criteria columns, then sort_by_indices.
    // nulls_first is accepted and ignored exactly like the reference does (:208).
    struct SortCriteria { std::string column; bool descending = false; bool nulls_first = false; };
    DataFrame sort(const std::vector<SortCriteria>& criteria) const {
        if (criteria.empty()) throw DataFrameError(DataFrameError::ComputeError, "Sort criteria cannot be empty");
        for (auto& c : criteria)
            if (column_by_name(c.column).data_type() == DataType::Utf8) return take(lexsort_indices(criteria));
        std::vector<rdf_array> cols;
        std::vector<rdf_sort_options> opts;
        bool host = true;   // host-resident criteria (the groups of a GROUP BY over a host-resident frame): the indices stay beside them
        for (auto& c : criteria) {
            for (auto& a : column_by_name(c.column).data().chunks()) { cols.push_back(a->view()); host &= a->host; }
            opts.push_back(rdf_sort_options{c.descending ? 1 : 0, 0});
        }
        auto idx = Array::make_out(DataType::UInt32, num_rows(), false, host);
        rdf_out ov = idx->out_view(num_rows());
        check(rdf_sort_to_indices(cols.data(), (int32_t)criteria.size(), (int64_t)num_chunks(), opts.data(), &ov));
        idx->length = ov.length;
        return take(idx);
    }
    // The criteria of a sort or a window as rdf_sort_key entries.  A numeric column goes by its chunks' views; a text column's
    // chunks go as offsets + bytes built from the mirror's strings, copied to the device when the frame's numeric columns
    // live there (one memory space per call, and the take that follows wants indices beside the columns).
    struct SortKeys {
        struct Text { std::vector<int32_t> offs; std::string bytes; std::vector<uint8_t> valid; std::vector<std::shared_ptr<DeviceBuffer>> dev; };
        std::vector<std::unique_ptr<Text>> keep;
        std::vector<std::vector<rdf_array>> num;
        std::vector<std::vector<rdf_utf8_array>> txt;
        std::vector<rdf_sort_key> keys;
    };
    bool numeric_columns_on_host() const {
        bool host = true;
        for (auto& c : columns_)
            if (c.data_type() != DataType::Utf8)
                for (auto& a : c.data().chunks()) host &= a->host;
        return host;
    }
    SortKeys sort_keys(const std::vector<SortCriteria>& criteria, bool host) const {
        const int32_t mem = host ? RDF_MEM_HOST : RDF_MEM_DEVICE;
        using Text = SortKeys::Text;
        SortKeys sk;
        sk.num.resize(criteria.size());
        sk.txt.resize(criteria.size());
        sk.keys.resize(criteria.size());
        auto place = [&](Text& t, const void* src, int64_t bytes) -> const void* {   // host bytes, or a device copy of them
            if (host) return src;
            t.dev.push_back(std::make_shared<DeviceBuffer>(bytes));
            if (bytes > 0) check(rdf_copy_h2d(t.dev.back()->data(), src, bytes));
            return t.dev.back()->data();
        };
        for (size_t k = 0; k < criteria.size(); ++k) {
            const Column& col = column_by_name(criteria[k].column);
            if (col.data_type() != DataType::Utf8) {
                for (auto& a : col.data().chunks()) sk.num[k].push_back(a->view());
            } else {
                for (auto& a : col.data().chunks()) {
                    sk.keep.push_back(std::make_unique<Text>());
                    Text& t = *sk.keep.back();
                    t.offs.reserve((size_t)a->length + 1);
                    t.offs.push_back(0);
                    for (int64_t r = 0; r < a->length; ++r) {
                        t.bytes += (*a->strings)[(size_t)(a->offset + r)];
                        if (t.bytes.size() > (size_t)INT32_MAX) throw DataFrameError(DataFrameError::ComputeError, "sort: a Utf8 chunk above 2^31-1 bytes");
                        t.offs.push_back((int32_t)t.bytes.size());
                    }
                    if (a->validity) t.valid = pack_bits(a->valid_to_host());
                    rdf_utf8_array u;
                    u.offsets.values = place(t, t.offs.data(), (int64_t)t.offs.size() * 4);
                    u.offsets.validity = t.valid.empty() ? nullptr : (const uint8_t*)place(t, t.valid.data(), (int64_t)t.valid.size());
                    u.offsets.offset = 0; u.offsets.length = a->length + 1; u.offsets.null_count = -1; u.offsets.dtype = RDF_I32; u.offsets.mem = mem;
                    u.data.values = place(t, t.bytes.data(), (int64_t)t.bytes.size());
                    u.data.validity = nullptr;
                    u.data.offset = 0; u.data.length = (int64_t)t.bytes.size(); u.data.null_count = 0; u.data.dtype = RDF_U8; u.data.mem = mem;
                    sk.txt[k].push_back(u);
                }
            }
            sk.keys[k].values = sk.num[k].empty() ? nullptr : sk.num[k].data();
            sk.keys[k].utf8 = sk.txt[k].empty() ? nullptr : sk.txt[k].data();
            sk.keys[k].options = rdf_sort_options{criteria[k].descending ? 1 : 0, 0};
        }
        return sk;
    }
    // lexsort_to_indices when a criterion is a Utf8 column (rdf_lexsort_to_indices: byte order, NULLs last, stable).
    ArrayRef lexsort_indices(const std::vector<SortCriteria>& criteria) const {
        const bool host = numeric_columns_on_host();
        const SortKeys sk = sort_keys(criteria, host);
        auto idx = Array::make_out(DataType::UInt32, num_rows(), false, host);
        rdf_out ov = idx->out_view(num_rows());
        check(rdf_lexsort_to_indices(sk.keys.data(), (int32_t)sk.keys.size(), (int64_t)num_chunks(), &ov));
        idx->length = ov.length;
        return idx;
    }
    // ---- membership: rdf_member_mask / rdf_first_occurrence as Boolean columns of this frame's chunking, and what is built on
    // them.  Float keys follow Spark (-0.0 == +0.0, NaN == NaN); Utf8 keys are byte strings.
    enum class Keep { First = RDF_KEEP_FIRST, Last = RDF_KEEP_LAST, None = RDF_KEEP_NONE };
    struct MaskOuts {   // one Boolean output per chunk
        std::vector<std::shared_ptr<Array>> arrays;
        std::vector<rdf_out> views;
        MaskOuts(const std::vector<int64_t>& rows, bool with_validity, bool host) {
            for (int64_t n : rows) { arrays.push_back(Array::make_out(DataType::Boolean, n, with_validity, host)); views.push_back(arrays.back()->out_view(n)); }
        }
        Column column(const std::string& name, size_t first, size_t count) {
            std::vector<ArrayRef> chunks;
            for (size_t i = first; i < first + count; ++i) { arrays[i]->length = views[i].length; arrays[i]->null_count = views[i].null_count; chunks.push_back(arrays[i]); }
            return Column::from_arrays(chunks, Field{name, DataType::Boolean, true});
        }
    };
    std::vector<int64_t> chunk_rows() const {
        std::vector<int64_t> rows;
        for (auto& a : columns_.at(0).data().chunks()) rows.push_back(a->length);
        return rows;
    }
    static void check_key_count(size_t n, const char* what) {
        if (n < 1 || n > (size_t)RDF_MEMBER_MAX_KEYS)
            throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": 1 to 4 key columns, got " + std::to_string(n) + " (more than 4 key columns are not supported)");
    }
    // SEMI / ANTI / IS_IN of this frame's rows against `other`'s: criteria[k].first of this frame pairs with .second of other
    Column member_mask(const DataFrame& other, const std::vector<std::pair<std::string, std::string>>& criteria, int32_t kind, const std::string& name) const {
        check_key_count(criteria.size(), "membership");
        std::vector<SortCriteria> lc, rc;
        for (auto& c : criteria) {
            if (column_by_name(c.first).data_type() != other.column_by_name(c.second).data_type()) throw DataFrameError(DataFrameError::ComputeError, "Join columns must have compatible types");
            lc.push_back(SortCriteria{c.first, false, false}); rc.push_back(SortCriteria{c.second, false, false});
        }
        const bool host = numeric_columns_on_host() && other.numeric_columns_on_host();
        const SortKeys lsk = sort_keys(lc, host), rsk = other.sort_keys(rc, host);
        MaskOuts out(chunk_rows(), kind == RDF_MEMBER_IS_IN, host);
        int64_t rows = 0;
        check(rdf_member_mask(lsk.keys.data(), (int64_t)num_chunks(), rsk.keys.data(), (int64_t)other.num_chunks(), (int32_t)criteria.size(), kind, out.views.data(), &rows));
        return out.column(name, 0, num_chunks());
    }
    // TRUE on the first / last / only row of every distinct tuple of the `subset` columns (all columns when empty)
    Column first_occurrence(const std::vector<std::string>& subset, Keep keep, const std::string& name) const {
        std::vector<SortCriteria> crit;
        if (subset.empty()) for (auto& c : columns_) crit.push_back(SortCriteria{c.name(), false, false});
        else for (auto& n : subset) crit.push_back(SortCriteria{n, false, false});
        check_key_count(crit.size(), "drop_duplicates");
        const bool host = numeric_columns_on_host();
        const SortKeys sk = sort_keys(crit, host);
        MaskOuts out(chunk_rows(), false, host);
        int64_t rows = 0;
        check(rdf_first_occurrence(sk.keys.data(), (int32_t)crit.size(), (int64_t)num_chunks(), (int32_t)keep, out.views.data(), &rows));
        return out.column(name, 0, num_chunks());
    }
    DataFrame drop_duplicates(const std::vector<std::string>& subset = {}, Keep keep = Keep::First) const { return filter_by_mask(first_occurrence(subset, keep, "\x01first")); }
    DataFrame distinct() const { return drop_duplicates(); }
    // INTERSECT / EXCEPT with SQL's DISTINCT set semantics (NULL equal to NULL), columns paired by position.  KEEP_FIRST over the
    // concatenation left-then-right marks the left rows that are the first of their tuple on the left (a); over right-then-left a
    // left row is TRUE only when no right row holds its tuple (b).  intersect = a AND NOT b, except = a AND b.
    DataFrame set_op(const DataFrame& other, bool intersect, const char* what) const {
        if (num_columns() != other.num_columns()) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": the frames differ in their number of columns");
        check_key_count(num_columns(), what);
        std::vector<SortCriteria> lc, rc;
        for (size_t k = 0; k < num_columns(); ++k) {
            if (columns_[k].data_type() != other.columns_[k].data_type()) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": column types differ");
            lc.push_back(SortCriteria{columns_[k].name(), false, false}); rc.push_back(SortCriteria{other.columns_[k].name(), false, false});
        }
        const bool host = numeric_columns_on_host() && other.numeric_columns_on_host();
        const SortKeys lsk = sort_keys(lc, host), rsk = other.sort_keys(rc, host);
        const size_t lnc = num_chunks(), rnc = other.num_chunks();
        std::vector<int64_t> lrows = chunk_rows(), rrows = other.chunk_rows();
        auto first_of = [&](bool left_first) -> Column {   // KEEP_FIRST over the two frames' chunks in the given order; -> the left part
            const SortKeys& a = left_first ? lsk : rsk; const SortKeys& b = left_first ? rsk : lsk;
            std::vector<std::vector<rdf_array>> num(lc.size());
            std::vector<std::vector<rdf_utf8_array>> txt(lc.size());
            std::vector<rdf_sort_key> keys(lc.size());
            for (size_t k = 0; k < lc.size(); ++k) {
                num[k] = a.num[k]; num[k].insert(num[k].end(), b.num[k].begin(), b.num[k].end());
                txt[k] = a.txt[k]; txt[k].insert(txt[k].end(), b.txt[k].begin(), b.txt[k].end());
                keys[k] = rdf_sort_key{num[k].empty() ? nullptr : num[k].data(), txt[k].empty() ? nullptr : txt[k].data(), rdf_sort_options{0, 0}};
            }
            std::vector<int64_t> rows = left_first ? lrows : rrows;
            const std::vector<int64_t>& tail = left_first ? rrows : lrows;
            rows.insert(rows.end(), tail.begin(), tail.end());
            MaskOuts out(rows, false, host);
            int64_t n = 0;
            check(rdf_first_occurrence(keys.data(), (int32_t)keys.size(), (int64_t)(lnc + rnc), RDF_KEEP_FIRST, out.views.data(), &n));
            return out.column(left_first ? "a" : "b", left_first ? 0 : rnc, lnc);
        };
        const DataFrame masks = DataFrame::from_columns({first_of(true), first_of(false)});
        const FilterRef b = BooleanFilter::column("b");
        return filter_by_mask(masks.evaluate_boolean_filter(BooleanFilter::and_(BooleanFilter::column("a"), intersect ? BooleanFilter::not_(b) : b)));
    }
    DataFrame intersect(const DataFrame& other) const { return set_op(other, true, "intersect"); }
    DataFrame except(const DataFrame& other) const { return set_op(other, false, "except"); }
    // rdf_groupby_sorted over columns of this frame: `groups` (0 .. 4 names) are the grouping columns, `value` the ONE column
    // the calls read (nullptr with no calls).  -> the group count, the UInt32 row index of every group's first row (groups in
    // ascending key order, NULL last) and one array per call: Int64 counts / sums, Float64 sums of a float column, UInt32 row
    // indices for first / last (with validity when ignore_nulls is set).  A capacity of the rows always suffices: one call.
    struct SortedGroups { int64_t groups = 0; ArrayRef group_rows; std::vector<ArrayRef> outs; };
    SortedGroups sorted_groups(const std::vector<std::string>& groups, const std::string* value, const std::vector<rdf_group_call>& calls) const {
        const bool host = numeric_columns_on_host();
        std::vector<SortCriteria> crit;
        for (auto& g : groups) crit.push_back(SortCriteria{g, false, false});
        if (value) crit.push_back(SortCriteria{*value, false, false});
        const SortKeys sk = sort_keys(crit, host);
        const int64_t cap = (int64_t)num_rows();
        const bool value_float = value && is_float(column_by_name(*value).data_type());
        auto rows = Array::make_out(DataType::UInt32, cap, false, host);
        rdf_out orow = rows->out_view(cap);
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& c : calls) {
            const DataType dt = c.fn == RDF_GRP_COUNT_DISTINCT ? DataType::Int64 : c.fn == RDF_GRP_SUM_DISTINCT ? (value_float ? DataType::Float64 : DataType::Int64) : DataType::UInt32;
            outs.push_back(Array::make_out(dt, cap, c.fn >= RDF_GRP_FIRST && c.ignore_nulls, host));
            ov.push_back(outs.back()->out_view(cap));
        }
        SortedGroups r;
        check(rdf_groupby_sorted(groups.empty() ? nullptr : sk.keys.data(), (int32_t)groups.size(), value ? &sk.keys[groups.size()] : nullptr, (int64_t)num_chunks(),
                                 calls.empty() ? nullptr : calls.data(), (int32_t)calls.size(), &orow, calls.empty() ? nullptr : ov.data(), &r.groups));
        rows->length = orow.length;
        r.group_rows = rows;
        for (size_t c = 0; c < outs.size(); ++c) {
            outs[c]->length = ov[c].length;
            outs[c]->null_count = ov[c].null_count;
            if (ov[c].null_count == 0) outs[c]->validity = nullptr;
            r.outs.push_back(outs[c]);
        }
        return r;
    }
    // rdf_groupby_percentile over columns of this frame: `groups` (0 .. 4 names) are the grouping columns, `value` the ONE
    // column the calls read.  -> the group count, the UInt32 row index of every group's first row (groups in ascending key
    // order, NULL last), one array per call — Float64 for RDF_PCT_CONT, UInt32 row indices into `value` for RDF_PCT_DISC, NULL
    // for a group without a non-NULL value — and the Int64 count of non-NULL values per group.  A capacity of the rows always
    // suffices (of one row without grouping columns): one call.  Without grouping columns a numeric column is answered by the radix select, no sort.
    struct PercentileGroups { int64_t groups = 0; ArrayRef group_rows, counts; std::vector<ArrayRef> outs; };
    PercentileGroups percentile_groups(const std::vector<std::string>& groups, const std::string& value, const std::vector<rdf_percentile_call>& calls) const {
        const bool host = numeric_columns_on_host();
        std::vector<SortCriteria> crit;
        for (auto& g : groups) crit.push_back(SortCriteria{g, false, false});
        crit.push_back(SortCriteria{value, false, false});
        const SortKeys sk = sort_keys(crit, host);
        const int64_t cap = groups.empty() ? std::min<int64_t>(1, (int64_t)num_rows()) : (int64_t)num_rows();   // no grouping columns: one row
        auto rows = Array::make_out(DataType::UInt32, cap, false, host), counts = Array::make_out(DataType::Int64, cap, false, host);
        rdf_out orow = rows->out_view(cap), ocnt = counts->out_view(cap);
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& c : calls) {
            outs.push_back(Array::make_out(c.kind == RDF_PCT_CONT ? DataType::Float64 : DataType::UInt32, cap, true, host));
            ov.push_back(outs.back()->out_view(cap));
        }
        PercentileGroups r;
        check(rdf_groupby_percentile(groups.empty() ? nullptr : sk.keys.data(), (int32_t)groups.size(), &sk.keys[groups.size()], (int64_t)num_chunks(),
                                     calls.empty() ? nullptr : calls.data(), (int32_t)calls.size(), &orow, calls.empty() ? nullptr : ov.data(), &ocnt, &r.groups));
        rows->length = orow.length;
        counts->length = ocnt.length;
        r.group_rows = rows;
        r.counts = counts;
        for (size_t c = 0; c < outs.size(); ++c) {
            outs[c]->length = ov[c].length;
            outs[c]->null_count = ov[c].null_count;
            if (ov[c].null_count == 0) outs[c]->validity = nullptr;
            r.outs.push_back(outs[c]);
        }
        return r;
    }
    // rdf_groupby_moments over columns of this frame: `groups` (0 .. 4 names) are the grouping columns, `x` the numeric column
    // the statistics are of — or, with `y`, the first of the pair.  calls[c].stat is an rdf_stat without y, an rdf_costat with
    // it.  -> the group count, the UInt32 row index of every group's first row (groups in ascending key order, NULL last),
    // one Float64 array per call — NULL where the statistic is absent: no counted row, a sample form of one row, a ratio over
    // M2 == 0 — and the Int64 count of counted rows per group.  The sort is over the grouping columns alone; a capacity of
    // the rows always suffices: one call.
    struct MomentGroups { int64_t groups = 0; ArrayRef group_rows, counts; std::vector<ArrayRef> outs; };
    MomentGroups moment_groups(const std::vector<std::string>& groups, const std::string& x, const std::string* y, const std::vector<rdf_group_stat_call>& calls) const {
        const bool host = numeric_columns_on_host();
        std::vector<SortCriteria> crit;
        for (auto& g : groups) crit.push_back(SortCriteria{g, false, false});
        const SortKeys sk = sort_keys(crit, host);
        const std::vector<rdf_array> xv = column_by_name(x).data().views();
        const std::vector<rdf_array> yv = y ? column_by_name(*y).data().views() : std::vector<rdf_array>();
        const int64_t cap = groups.empty() ? std::min<int64_t>(1, (int64_t)num_rows()) : (int64_t)num_rows();   // no grouping columns: one row
        auto rows = Array::make_out(DataType::UInt32, cap, false, host), counts = Array::make_out(DataType::Int64, cap, false, host);
        rdf_out orow = rows->out_view(cap), ocnt = counts->out_view(cap);
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t c = 0; c < calls.size(); ++c) {
            outs.push_back(Array::make_out(DataType::Float64, cap, true, host));
            ov.push_back(outs.back()->out_view(cap));
        }
        MomentGroups r;
        check(rdf_groupby_moments(groups.empty() ? nullptr : sk.keys.data(), (int32_t)groups.size(), xv.data(), y ? yv.data() : nullptr, (int64_t)num_chunks(),
                                  calls.empty() ? nullptr : calls.data(), (int32_t)calls.size(), &orow, calls.empty() ? nullptr : ov.data(), &ocnt, nullptr, 0, &r.groups));
        rows->length = orow.length;
        counts->length = ocnt.length;
        r.group_rows = rows;
        r.counts = counts;
        for (size_t c = 0; c < outs.size(); ++c) {
            outs[c]->length = ov[c].length;
            outs[c]->null_count = ov[c].null_count;
            if (ov[c].null_count == 0) outs[c]->validity = nullptr;
            r.outs.push_back(outs[c]);
        }
        return r;
    }
    // rdf_groupby_collect over columns of this frame: `groups` (0 .. 4 names) are the grouping columns, `value` the ONE column
    // collected, kind RDF_COLLECT_LIST / RDF_COLLECT_SET.  -> the group and element counts, the UInt32 row index of every
    // group's first row (groups in ascending key order, NULL last), the Int32 offsets (groups + 1 entries), the UInt32 row
    // index of every element and, for a numeric value column, the elements themselves (nullptr for Utf8).  A capacity of
    // the rows always suffices: one call.  A frame without rows gives empty arrays and offsets of the one entry 0.
    struct CollectedGroups { int64_t groups = 0, elements = 0; ArrayRef group_rows, offsets, child_rows, values; };
    CollectedGroups collected_groups(const std::vector<std::string>& groups, const std::string& value, int32_t kind) const {
        const bool host = numeric_columns_on_host();
        std::vector<SortCriteria> crit;
        for (auto& g : groups) crit.push_back(SortCriteria{g, false, false});
        crit.push_back(SortCriteria{value, false, false});
        const SortKeys sk = sort_keys(crit, host);
        const int64_t cap = (int64_t)num_rows();
        const DataType vdt = column_by_name(value).data_type();
        CollectedGroups r;
        if (cap == 0) {
            r.group_rows = Array::from_vec<uint32_t>({});
            r.offsets = Array::from_vec<int32_t>({0});
            r.child_rows = Array::from_vec<uint32_t>({});
            if (vdt != DataType::Utf8) { auto v = Array::make_out(vdt, 0, false, host); r.values = v; }
            return r;
        }
        auto rows = Array::make_out(DataType::UInt32, cap, false, host), offs = Array::make_out(DataType::Int32, cap + 1, false, host);
        auto child = Array::make_out(DataType::UInt32, cap, false, host);
        auto vals = vdt == DataType::Utf8 ? nullptr : Array::make_out(vdt, cap, false, host);
        rdf_out orow = rows->out_view(cap), ooff = offs->out_view(cap + 1), ochild = child->out_view(cap), oval{};
        if (vals) oval = vals->out_view(cap);
        check(rdf_groupby_collect(groups.empty() ? nullptr : sk.keys.data(), (int32_t)groups.size(), &sk.keys[groups.size()], (int64_t)num_chunks(), kind,
                                  &orow, &ooff, &ochild, vals ? &oval : nullptr, &r.groups, &r.elements));
        rows->length = orow.length; offs->length = ooff.length; child->length = ochild.length;
        if (vals) vals->length = oval.length;
        r.group_rows = rows; r.offsets = offs; r.child_rows = child; r.values = vals;
        return r;
    }
    // sort_by_indices (:216-222): Column::take of every column (chunk size 4096 as in the reference)
    DataFrame take(const ArrayRef& indices) const {
        std::vector<Column> cols;
        for (auto& c : columns_) cols.push_back(c.take(indices, 4096));
        return DataFrame(schema_, std::move(cols));
    }

    // Window functions (the reference declares them with empty bodies: WindowSpec in src/window.rs, row_number .. lead in
    // src/functions/window.rs, ntile in src/functions/scalar.rs:345; the semantics are SQL's, written down at rdf_window).
    // partition_by: rows that agree on every listed column form a partition (NULL is a value); order_by: the order inside a
    // partition, NULLs last, ties in row order.  rows_between / range_between set the frame of with_window_agg; with_window
    // ignores it (ranks have no frame in SQL).
    enum class WindowFunction : int32_t {
        RowNumber = RDF_WIN_ROW_NUMBER, Rank = RDF_WIN_RANK, DenseRank = RDF_WIN_DENSE_RANK, PercentRank = RDF_WIN_PERCENT_RANK,
        CumeDist = RDF_WIN_CUME_DIST, Ntile = RDF_WIN_NTILE, Lag = RDF_WIN_LAG, Lead = RDF_WIN_LEAD
    };
    class WindowSpec {
      public:
        WindowSpec& partition_by(std::vector<std::string> cols) { partition_ = std::move(cols); return *this; }
        WindowSpec& order_by(std::vector<SortCriteria> criteria) { order_ = std::move(criteria); return *this; }
        // The frame, in the reference's spelling (src/window.rs): unbounded_preceding / unbounded_following, 0 = current_row, a
        // negative number = that many rows preceding, a positive one = following.  range_between takes no offsets.
        static constexpr int64_t unbounded_preceding = INT64_MIN, current_row = 0, unbounded_following = INT64_MAX;
        WindowSpec& rows_between(int64_t start, int64_t end) { frame_ = make_frame(RDF_FRAME_ROWS, start, end); by_ = 0; return *this; }
        WindowSpec& range_between(int64_t start, int64_t end) { frame_ = make_frame(RDF_FRAME_RANGE, start, end); by_ = 0; return *this; }
        // RANGE BETWEEN with offsets in the ORDER KEY's units (Spark's rangeBetween over a numeric column): range_by(-7, 0) over a
        // day-number column is a rolling 7-day frame.  rows_between's sign convention; the integer form is for Int32 / Int64 order
        // columns (dates and timestamps as their storage) and takes the unbounded_* sentinels, the double form is for Float64
        // ones: finite offsets, -infinity / +infinity = unbounded preceding / following (a double has no spare sentinel, and the
        // C ABI itself refuses an infinite OFFSET: here an infinity is never an offset, it names the unbounded kind).  Exactly one order column; with_window_agg sends such a spec through rdf_window_range_agg.
        WindowSpec& range_by(int64_t start, int64_t end) {
            const rdf_window_frame f = make_frame(RDF_FRAME_RANGE, start, end);
            range_ = rdf_window_range_frame{f.start_kind, f.end_kind, f.start, f.end, 0.0, 0.0};
            by_ = 1;
            return *this;
        }
        WindowSpec& range_by(double start, double end) {
            auto bound = [](double b, int32_t* kind, double* off) {
                *off = 0.0;
                if (b == -std::numeric_limits<double>::infinity()) *kind = RDF_BOUND_UNBOUNDED_PRECEDING;
                else if (b == std::numeric_limits<double>::infinity()) *kind = RDF_BOUND_UNBOUNDED_FOLLOWING;
                else if (b == 0.0) *kind = RDF_BOUND_CURRENT_ROW;
                else { *kind = b < 0.0 ? RDF_BOUND_PRECEDING : RDF_BOUND_FOLLOWING; *off = b < 0.0 ? -b : b; }   // (a NaN offset stays NaN and is refused by the library)
            };
            range_ = rdf_window_range_frame{0, 0, 0, 0, 0.0, 0.0};
            bound(start, &range_.start_kind, &range_.start_f);
            bound(end, &range_.end_kind, &range_.end_f);
            by_ = 2;
            return *this;
        }
        template <class A, class B, class = typename std::enable_if<std::is_integral<A>::value && std::is_integral<B>::value &&
                                                                     !(std::is_same<A, int64_t>::value && std::is_same<B, int64_t>::value)>::type>
        WindowSpec& range_by(A start, B end) { return range_by((int64_t)start, (int64_t)end); }   // (int literals: not ambiguous between the two forms)
        int range_by_form() const { return by_; }      // 0: no range_by frame, 1: integer offsets, 2: double offsets
        const rdf_window_range_frame& range_frame() const { return range_; }
        const std::vector<std::string>& partition() const { return partition_; }
        const std::vector<SortCriteria>& order() const { return order_; }
        // no frame set: SQL's default, RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW
        const rdf_window_frame& frame() const { return frame_; }
      private:
        static rdf_window_frame make_frame(int32_t unit, int64_t start, int64_t end) {
            auto bound = [](int64_t b, int32_t* kind, int64_t* off) {
                *off = 0;
                if (b == unbounded_preceding) *kind = RDF_BOUND_UNBOUNDED_PRECEDING;
                else if (b == unbounded_following) *kind = RDF_BOUND_UNBOUNDED_FOLLOWING;
                else if (b == 0) *kind = RDF_BOUND_CURRENT_ROW;
                else { *kind = b < 0 ? RDF_BOUND_PRECEDING : RDF_BOUND_FOLLOWING; *off = b < 0 ? -b : b; }
            };
            rdf_window_frame f{unit, 0, 0, 0, 0, 0};
            bound(start, &f.start_kind, &f.start);
            bound(end, &f.end_kind, &f.end);
            return f;
        }
        std::vector<std::string> partition_;
        std::vector<SortCriteria> order_;
        rdf_window_frame frame_{RDF_FRAME_RANGE, RDF_BOUND_UNBOUNDED_PRECEDING, RDF_BOUND_CURRENT_ROW, 0, 0, 0};
        rdf_window_range_frame range_{RDF_BOUND_UNBOUNDED_PRECEDING, RDF_BOUND_CURRENT_ROW, 0, 0, 0.0, 0.0};
        int by_ = 0;
    };
    enum class WindowAggregate : int32_t {
        Sum = RDF_WAGG_SUM, Min = RDF_WAGG_MIN, Max = RDF_WAGG_MAX, Count = RDF_WAGG_COUNT, Avg = RDF_WAGG_AVG,
        FirstValue = RDF_WAGG_FIRST_VALUE, LastValue = RDF_WAGG_LAST_VALUE
    };
    // Appends fn over `spec` as column `name`, chunked like the frame: Int64 for RowNumber / Rank / DenseRank / Ntile(param
    // buckets), Float64 for PercentRank / CumeDist; Lag / Lead(param rows) append `value_column` of the row param places
    // before / after in the partition — any dtype, text included — NULL where the partition ends (rdf_window hands out row
    // indices, Column::take gathers through them: a NULL index is a NULL row).
    DataFrame with_window(const std::string& name, const WindowSpec& spec, WindowFunction fn, int64_t param = 0,
                          const std::string& value_column = "") const {
        const bool shifts = fn == WindowFunction::Lag || fn == WindowFunction::Lead;
        if (shifts && value_column.empty()) throw DataFrameError(DataFrameError::ComputeError, "with_window: lag / lead need a value column");
        const bool host = numeric_columns_on_host();
        std::vector<SortCriteria> part;
        for (auto& c : spec.partition()) part.push_back(SortCriteria{c, false, false});
        const SortKeys pk = sort_keys(part, host), ok = sort_keys(spec.order(), host);
        const DataType dt = shifts ? DataType::UInt32 : (fn == WindowFunction::PercentRank || fn == WindowFunction::CumeDist) ? DataType::Float64 : DataType::Int64;
        auto out = Array::make_out(dt, num_rows(), shifts, host);
        rdf_out ov = out->out_view(num_rows());
        const rdf_window_call call{(int32_t)fn, 0, param};
        const bool keyed = !pk.keys.empty() || !ok.keys.empty();
        check(rdf_window(pk.keys.empty() ? nullptr : pk.keys.data(), (int32_t)pk.keys.size(), ok.keys.empty() ? nullptr : ok.keys.data(),
                         (int32_t)ok.keys.size(), (int64_t)num_chunks(), keyed ? 0 : num_rows(), &call, 1, &ov));
        out->length = ov.length;
        out->null_count = ov.null_count;
        ArrayRef whole = out;
        Field field{name, dt, false};
        if (shifts) {
            const Column taken = column_by_name(value_column).take(out, 4096);
            whole = taken.data().chunk(0);
            field = Field{name, taken.data_type(), true};
        }
        std::vector<ArrayRef> chunks;                       // one array of all rows -> the frame's batches, zero-copy
        int64_t at = 0;
        for (int64_t len : columns_.at(0).data().chunk_counts()) { chunks.push_back(whole->slice(at, len)); at += len; }
        return with_column(name, Column::from_arrays(std::move(chunks), field));
    }
    // Appends fn of `value_column` over the frame of `spec` as column `name`, chunked like the frame (rdf_window_agg): Sum / Min /
    // Max of an Int64 or Float64 column in its own type, Avg as Float64, Count as Int64 (an empty value_column counts the
    // frame's rows); NULL where the frame holds no valid row, except Count.  FirstValue / LastValue append `value_column` — any
    // dtype, text included — of the frame's first / last row, NULL where the frame is empty (row indices gathered by Column::take).
    DataFrame with_window_agg(const std::string& name, const WindowSpec& spec, WindowAggregate fn, const std::string& value_column = "") const {
        const bool picks = fn == WindowAggregate::FirstValue || fn == WindowAggregate::LastValue;
        if (value_column.empty() && fn != WindowAggregate::Count) throw DataFrameError(DataFrameError::ComputeError, "with_window_agg: a value column is needed");
        const bool host = numeric_columns_on_host();
        std::vector<SortCriteria> part;
        for (auto& c : spec.partition()) part.push_back(SortCriteria{c, false, false});
        const SortKeys pk = sort_keys(part, host), ok = sort_keys(spec.order(), host);
        const bool reads = !picks && !value_column.empty();
        std::vector<rdf_array> vchunks;
        DataType vdt = DataType::Int64;
        if (reads) {
            const Column& vc = column_by_name(value_column);
            vdt = vc.data_type();
            if (vdt != DataType::Int64 && vdt != DataType::Float64) throw DataFrameError(DataFrameError::ComputeError, "with_window_agg: Int64 or Float64 value columns");
            for (auto& a : vc.data().chunks()) vchunks.push_back(a->view());
        }
        const rdf_array* vptr = vchunks.data();
        const DataType dt = picks ? DataType::UInt32 : fn == WindowAggregate::Count ? DataType::Int64 : fn == WindowAggregate::Avg ? DataType::Float64 : vdt;
        const bool nullable = fn != WindowAggregate::Count;
        auto out = Array::make_out(dt, num_rows(), nullable, host);
        rdf_out ov = out->out_view(num_rows());
        if (spec.range_by_form() != 0) {                    // offsets in the order key's units: one numeric order column of the form's type
            if (spec.order().size() != 1) throw DataFrameError(DataFrameError::ComputeError, "with_window_agg: range_by needs exactly one order column");
            const DataType kdt = column_by_name(spec.order()[0].column).data_type();
            const bool fits = spec.range_by_form() == 1 ? (kdt == DataType::Int32 || kdt == DataType::Int64) : kdt == DataType::Float64;
            if (!fits) throw DataFrameError(DataFrameError::ComputeError, std::string("with_window_agg: range_by with ") +
                                            (spec.range_by_form() == 1 ? "integer offsets needs an Int32 / Int64" : "double offsets needs a Float64") +
                                            " order column, not " + type_name(kdt));
            const rdf_window_range_call rcall{(int32_t)fn, reads ? 0 : -1, spec.range_frame()};
            check(rdf_window_range_agg(pk.keys.empty() ? nullptr : pk.keys.data(), (int32_t)pk.keys.size(), ok.keys.data(), 1,
                                       reads ? &vptr : nullptr, reads ? 1 : 0, (int64_t)num_chunks(), &rcall, 1, &ov));
        } else {
            const rdf_window_agg_call call{(int32_t)fn, reads ? 0 : -1, spec.frame()};
            const bool keyed = !pk.keys.empty() || !ok.keys.empty() || reads;
            check(rdf_window_agg(pk.keys.empty() ? nullptr : pk.keys.data(), (int32_t)pk.keys.size(), ok.keys.empty() ? nullptr : ok.keys.data(),
                                 (int32_t)ok.keys.size(), reads ? &vptr : nullptr, reads ? 1 : 0, (int64_t)num_chunks(), keyed ? 0 : num_rows(), &call, 1, &ov));
        }
        out->length = ov.length;
        out->null_count = ov.null_count;
        ArrayRef whole = out;
        Field field{name, dt, nullable};
        if (picks) {
            const Column taken = column_by_name(value_column).take(out, 4096);
            whole = taken.data().chunk(0);
            field = Field{name, taken.data_type(), true};
        }
        std::vector<ArrayRef> chunks;                       // one array of all rows -> the frame's batches, zero-copy
        int64_t at = 0;
        for (int64_t len : columns_.at(0).data().chunk_counts()) { chunks.push_back(whole->slice(at, len)); at += len; }
        return with_column(name, Column::from_arrays(std::move(chunks), field));
    }

  private:
    Schema schema_;
    std::vector<Column> columns_;
};

using WindowSpec = DataFrame::WindowSpec;           // the reference's names (src/window.rs, src/functions/window.rs)
using WindowFunction = DataFrame::WindowFunction;
using WindowAggregate = DataFrame::WindowAggregate;

// ------------------------------------------------------------------------------------------------
// GpuFrame: a DataFrame of numeric columns pinned in HBM behind a frame handle (rdf_frame_pin), and the reference's
// frame-producing operators — DataFrame::filter (src/dataframe.rs:178-189), DataFrame::take / sort (:194-222), GroupAggregate —
// as handle-in / handle-out calls: nothing per RecordBatch is marshalled, so a frame held in the readers' 1024-row batches
// costs what its kernels cost, and a chain df.pin().filter(..).sort(..) never leaves the device.  to_dataframe() materialises
// the columns (one descriptor walk) when a caller wants Arrow arrays back; they alias the frame's buffers and keep it alive.
class GpuFrame {
  public:
    static GpuFrame pin(const DataFrame& df) {
        if (df.num_columns() == 0 || df.num_chunks() == 0) throw DataFrameError(DataFrameError::ComputeError, "cannot pin an empty frame");
        std::vector<rdf_array> views;
        for (size_t c = 0; c < df.num_columns(); ++c) {
            const DataType dt = df.column(c).data_type();
            if (dt == DataType::Utf8 || dt == DataType::Boolean) throw DataFrameError(DataFrameError::ComputeError, "GpuFrame holds numeric columns (column " + df.column(c).name() + ")");
            for (auto& a : df.column(c).data().chunks()) views.push_back(a->view());
        }
        rdf_frame* h = nullptr;
        check(rdf_frame_pin(views.data(), (int32_t)df.num_columns(), (int64_t)df.num_chunks(), &h));
        GpuFrame g;
        g.schema_ = df.schema();
        g.h_ = std::shared_ptr<Handle>(new Handle{h, std::make_shared<DataFrame>(df)});   // the pinned buffers live as long as the handle
        return g;
    }
    const Schema& schema() const { return schema_; }
    size_t num_columns() const { return schema_.fields.size(); }
    int64_t num_rows() const { int64_t r = 0; check(rdf_frame_info(h_->h, nullptr, nullptr, &r)); return r; }
    int64_t num_chunks() const { int64_t c = 0; check(rdf_frame_info(h_->h, nullptr, &c, nullptr)); return c; }

    // DataFrame::filter: the predicate over every batch, every column compacted in one pass, batch boundaries kept
    GpuFrame filter(const FilterRef& condition) const {
        Lowered low;
        for (auto& f : schema_.fields) low.columns.push_back(f.name);     // expression column c = frame column c
        const int root = low.add(filter_to_expr(condition, [this](const std::string& n) {
            if (!schema_.column_with_name(n)) throw DataFrameError(DataFrameError::ComputeError, "Cannot find column " + n);
            return Expr::col(n);
        }));
        rdf_frame* out = nullptr;
        check(rdf_filter_frame(h_->h, low.nodes.data(), (int32_t)low.nodes.size(), root, &out));
        return derived(out, schema_);
    }
    // DataFrame::take / sort_by_indices: every column gathered by one index list in one pass -> one batch per column
    GpuFrame take(const ArrayRef& indices) const {
        const rdf_array idx = indices->view();
        rdf_frame* out = nullptr;
        check(rdf_take_frame(h_->h, &idx, &out));
        return derived(out, nullable_schema());
    }
    // DataFrame::sort: lexsort_to_indices over the criteria columns, then the take of every column by that order
    GpuFrame sort(const std::vector<DataFrame::SortCriteria>& criteria) const {
        if (criteria.empty()) throw DataFrameError(DataFrameError::ComputeError, "Sort criteria cannot be empty");
        std::vector<int32_t> cols;
        std::vector<rdf_sort_options> opts;
        for (auto& c : criteria) {
            const auto f = schema_.column_with_name(c.column);
            if (!f) throw DataFrameError(DataFrameError::ComputeError, "Cannot find column " + c.column);
            cols.push_back((int32_t)f->first);
            opts.push_back(rdf_sort_options{c.descending ? 1 : 0, 0});
        }
        rdf_frame* out = nullptr;
        check(rdf_sort_frame(h_->h, cols.data(), (int32_t)cols.size(), opts.data(), nullptr, &out));
        return derived(out, schema_);
    }
    // GroupAggregate(groups, [one aggregation]) -> columns: the grouping columns, "<fn>(<value>)", "count"
    GpuFrame group_aggregate(const std::vector<std::string>& groups, const std::string& value, plan::AggregateFunction fn, int64_t max_groups) const {
        using AF = plan::AggregateFunction;
        std::vector<int32_t> keys;
        Schema s;
        for (auto& g : groups) {
            const auto f = schema_.column_with_name(g);
            if (!f) throw DataFrameError(DataFrameError::ComputeError, "Grouping column " + g + " does not exist");
            keys.push_back((int32_t)f->first);
            s.fields.push_back(f->second);
        }
        int32_t vcol = -1;
        DataType vdt = DataType::Int64;
        if (fn != AF::Count) {
            const auto f = schema_.column_with_name(value);
            if (!f) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column " + value + " does not exist");
            vcol = (int32_t)f->first; vdt = f->second.data_type;
        }
        if (fn == AF::Avg) throw DataFrameError(DataFrameError::ComputeError, "avg = sum / count on the caller's side");
        const int32_t agg = fn == AF::Sum ? RDF_AGG_SUM : fn == AF::Min ? RDF_AGG_MIN : fn == AF::Max ? RDF_AGG_MAX : RDF_AGG_COUNT;
        const bool fl = vdt == DataType::Float32 || vdt == DataType::Float64;
        const DataType odt = fn == AF::Count ? DataType::Int64 : fl ? DataType::Float64 : (agg != RDF_AGG_SUM && vdt == DataType::UInt64) ? DataType::UInt64 : DataType::Int64;
        const char* names[] = {"sum", "min", "max", "count"};
        s.fields.push_back(Field{std::string(names[agg]) + "(" + (fn == AF::Count ? std::string("*") : value) + ")", odt, true});
        s.fields.push_back(Field{"count", DataType::Int64, false});
        rdf_frame* out = nullptr;
        check(rdf_groupby_agg_frame(h_->h, keys.data(), (int32_t)keys.size(), vcol, agg, max_groups, &out));
        return derived(out, s);
    }
    // AggregateFunctions over a column of the pinned frame (sum / min / max / count in one fused pass)
    rdf_agg_result aggregate(const std::string& column) const {
        const auto f = schema_.column_with_name(column);
        if (!f) throw DataFrameError(DataFrameError::ComputeError, "Cannot find column " + column);
        if (num_columns() > 8) throw DataFrameError(DataFrameError::ComputeError, "programs run over frames of at most 8 columns: select first");
        rdf_expr_node n;
        std::memset(&n, 0, sizeof n);
        n.kind = RDF_NODE_COLUMN; n.column = (int32_t)f->first; n.lhs = n.rhs = -1;
        rdf_program p;
        std::memset(&p, 0, sizeof p);
        p.nodes = &n; p.nnodes = 1; p.filter_root = -1; p.nvalues = 1; p.value_roots[0] = 0; p.sink = RDF_SINK_AGG;
        rdf_agg_result r;
        check(rdf_pipeline_frame(&p, h_->h, nullptr, &r));
        return r;
    }
    // Arrow arrays back: one descriptor walk; the arrays alias the frame's buffers and keep the handle alive
    DataFrame to_dataframe() const {
        int32_t nc = 0; int64_t nch = 0, rows = 0;
        check(rdf_frame_info(h_->h, &nc, &nch, &rows));
        std::vector<Column> cols;
        std::vector<rdf_array> views((size_t)std::max<int64_t>(nch, 1));
        for (int32_t c = 0; c < nc; ++c) {
            check(rdf_frame_column(h_->h, c, views.data()));
            std::vector<ArrayRef> chunks;
            for (int64_t i = 0; i < nch; ++i) {
                auto a = std::make_shared<Array>();
                a->dtype = schema_.fields[(size_t)c].data_type;
                a->offset = views[(size_t)i].offset;
                a->length = views[(size_t)i].length;
                a->values = std::make_shared<DeviceBuffer>(const_cast<void*>(views[(size_t)i].values), a->length * (int64_t)type_size(a->dtype), h_);
                if (views[(size_t)i].validity) {
                    a->validity = std::make_shared<DeviceBuffer>(const_cast<uint8_t*>(views[(size_t)i].validity), (a->offset + a->length + 7) / 8, h_);
                    int64_t valid = 0; int32_t some = 0;
                    const rdf_array one = a->view_unknown_nulls();
                    check(rdf_count(&one, 1, &valid, &some));
                    a->null_count = a->length - valid;
                }
                chunks.push_back(a);
            }
            cols.push_back(Column::from_arrays(chunks, schema_.fields[(size_t)c]));
        }
        return DataFrame::from_columns(std::move(cols));
    }

  private:
    friend class ShardedFrame;
    struct Handle { rdf_frame* h; std::shared_ptr<DataFrame> pinned; ~Handle() { if (h) (void)rdf_frame_release(h); } };
    Schema schema_;
    std::shared_ptr<Handle> h_;
    GpuFrame derived(rdf_frame* out, const Schema& s) const {
        GpuFrame g;
        g.schema_ = s;
        g.h_ = std::shared_ptr<Handle>(new Handle{out, nullptr});      // the new frame owns its buffers
        return g;
    }
    Schema nullable_schema() const { Schema s = schema_; for (auto& f : s.fields) f.nullable = true; return s; }
};

// ------------------------------------------------------------------------------------------------
// ShardedFrame: one rank's shard of a DataFrame whose RecordBatches are spread over the GPUs of a node by row ranges
//  — the N-GPU form of what LazyFrame::evaluate (src/lazyframe.rs:311-315) drives.  Every reference kernel is
// per-chunk independent, so filter / take-within-shard / elementwise steps are the GpuFrame's own (no communication: the
// outputs stay sharded in rank order); AggregateFunctions fold the ranks' partials (rdf_agg_combine) and GroupAggregate — the
// panic! at src/evaluation.rs:73 — runs the library's exchange (rdf_groupby_agg_frame_dist: local aggregate, partial groups or
// rows to their owners over RCCL / peer copies, merge).  One ShardedFrame per rank, used by the thread that drives its GPU.
class Communicator {
  public:
    // one process (or thread) per GPU: rank 0 makes the id (unique_id()) and hands it to the others
    static std::array<uint8_t, RDF_COMM_ID_BYTES> unique_id() { std::array<uint8_t, RDF_COMM_ID_BYTES> id{}; check(rdf_comm_unique_id(id.data())); return id; }
    static std::shared_ptr<Communicator> init_rank(int world, int rank, const std::array<uint8_t, RDF_COMM_ID_BYTES>& id) {
        rdf_comm* c = nullptr;
        check(rdf_comm_init_rank(world, rank, id.data(), &c));
        return std::shared_ptr<Communicator>(new Communicator(c));
    }
    // a single process driving every GPU: communicator i belongs to the thread that called rdf_set_device(devices[i])
    static std::vector<std::shared_ptr<Communicator>> init_all(const std::vector<int32_t>& devices, rdf_comm_kind kind = RDF_COMM_RCCL) {
        std::vector<rdf_comm*> raw(devices.size(), nullptr);
        check(rdf_comm_init_all((int32_t)devices.size(), devices.data(), kind, raw.data()));
        std::vector<std::shared_ptr<Communicator>> out;
        for (rdf_comm* c : raw) out.push_back(std::shared_ptr<Communicator>(new Communicator(c)));
        return out;
    }
    ~Communicator() { if (c_) (void)rdf_comm_destroy(c_); }
    Communicator(const Communicator&) = delete;
    Communicator& operator=(const Communicator&) = delete;
    int world() const { int32_t w = 1; check(rdf_comm_info(c_, &w, nullptr, nullptr, nullptr, nullptr)); return w; }
    int rank() const { int32_t r = 0; check(rdf_comm_info(c_, nullptr, &r, nullptr, nullptr, nullptr)); return r; }
    void barrier() const { check(rdf_comm_barrier(c_)); }
    rdf_comm* raw() const { return c_; }

  private:
    explicit Communicator(rdf_comm* c) : c_(c) {}
    rdf_comm* c_;
};

class ShardedFrame {
  public:
    ShardedFrame(GpuFrame local, std::shared_ptr<Communicator> comm) : local_(std::move(local)), comm_(std::move(comm)) {}
    const GpuFrame& local() const { return local_; }
    const Communicator& comm() const { return *comm_; }
    // shard-local operators: row order across ranks = rank order
    ShardedFrame filter(const FilterRef& condition) const { return ShardedFrame(local_.filter(condition), comm_); }
    // rows of the whole frame
    int64_t num_rows() const {
        int64_t mine = local_.num_rows(), total = 0;
        std::vector<int64_t> all((size_t)comm_->world());
        check(rdf_comm_allgather(comm_->raw(), &mine, 8, all.data()));
        for (int64_t x : all) total += x;
        return total;
    }
    // AggregateFunctions::{sum, min, max, count} of a column over ALL shards: identical bits on every rank
    rdf_agg_result aggregate(const std::string& column) const {
        rdf_agg_result r = local_.aggregate(column);
        check(rdf_agg_combine(comm_->raw(), &r, 1));
        return r;
    }
    // GroupAggregate(groups = [one Int64 / UInt64 column], [one aggregation]) over all shards -> the groups THIS rank owns
    // (the union over the ranks is the result; owner = hash(key) % world); columns: key, "<fn>(<value>)", "count"
    GpuFrame group_aggregate(const std::string& group, const std::string& value, plan::AggregateFunction fn, int64_t max_groups,
                             rdf_exchange_mode exchange = RDF_EXCHANGE_AUTO, rdf_exchange_stats* stats = nullptr) const {
        using AF = plan::AggregateFunction;
        const Schema& sc = local_.schema();
        const auto kf = sc.column_with_name(group);
        if (!kf) throw DataFrameError(DataFrameError::ComputeError, "Grouping column " + group + " does not exist");
        if (fn == AF::Avg) throw DataFrameError(DataFrameError::ComputeError, "avg = sum / count on the caller's side");
        int32_t vcol = -1;
        DataType vdt = DataType::Int64;
        if (fn != AF::Count) {
            const auto f = sc.column_with_name(value);
            if (!f) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column " + value + " does not exist");
            vcol = (int32_t)f->first; vdt = f->second.data_type;
        }
        const int32_t agg = fn == AF::Sum ? RDF_AGG_SUM : fn == AF::Min ? RDF_AGG_MIN : fn == AF::Max ? RDF_AGG_MAX : RDF_AGG_COUNT;
        const bool fl = vdt == DataType::Float32 || vdt == DataType::Float64;
        const DataType odt = fn == AF::Count ? DataType::Int64 : fl ? DataType::Float64 : (agg != RDF_AGG_SUM && vdt == DataType::UInt64) ? DataType::UInt64 : DataType::Int64;
        const char* names[] = {"sum", "min", "max", "count"};
        Schema s;
        s.fields.push_back(kf->second);
        s.fields.push_back(Field{std::string(names[agg]) + "(" + (fn == AF::Count ? std::string("*") : value) + ")", odt, true});
        s.fields.push_back(Field{"count", DataType::Int64, false});
        rdf_frame* out = nullptr;
        check(rdf_groupby_agg_frame_dist(comm_->raw(), local_.h_->h, (int32_t)kf->first, vcol, agg, max_groups, exchange, &out, stats));
        return local_.derived(out, s);
    }

  private:
    GpuFrame local_;
    std::shared_ptr<Communicator> comm_;
};

// ------------------------------------------------------------------------------------------------
// ScalarFunctions / AggregateFunctions over device columns (chunk list in, chunk list out)

struct ListArray;

struct ScalarFunctions {
    // explode (src/functions/scalar.rs:237, declared with an empty body: Spark's semantics, written down at rdf_list_explode).
    // `list` has one row per row of `frame`.  Every element of every non-NULL list becomes one row: every column of `frame`
    // taken by the element's list row, then the element column `name`, taken from the list's child.  outer (explode_outer):
    // a NULL or empty list keeps its row, with a NULL element.  posexplode adds the 0-based position inside the list as the
    // Int32 column `pos_name` in front of the element column (NULL where the element is).  Defined below ListArray.
    static inline DataFrame explode(const DataFrame& frame, const ListArray& list, const std::string& name, bool outer = false);
    static inline DataFrame explode_outer(const DataFrame& frame, const ListArray& list, const std::string& name);
    static inline DataFrame posexplode(const DataFrame& frame, const ListArray& list, const std::string& pos_name, const std::string& name, bool outer = false);
    static std::vector<ArrayRef> binary(int32_t op, const std::vector<ArrayRef>& left, const std::vector<ArrayRef>& right) {
        if (left.size() != right.size()) throw DataFrameError(DataFrameError::ComputeError, "chunk lists differ in length");
        std::vector<rdf_array> a, b;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t i = 0; i < left.size(); ++i) {
            a.push_back(left[i]->view()); b.push_back(right[i]->view());
            outs.push_back(Array::make_out(left[i]->dtype, left[i]->length, left[i]->validity || right[i]->validity, left[i]->host));
            ov.push_back(outs.back()->out_view(left[i]->length));
        }
        check(rdf_binary(op, a.data(), b.data(), (int64_t)a.size(), ov.data()));
        return finish(outs, ov);
    }
    static std::vector<ArrayRef> unary(int32_t op, const std::vector<ArrayRef>& arr) {
        std::vector<rdf_array> a;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& x : arr) { a.push_back(x->view()); outs.push_back(Array::make_out(x->dtype, x->length, x->validity != nullptr, x->host)); ov.push_back(outs.back()->out_view(x->length)); }
        check(rdf_unary(op, a.data(), (int64_t)a.size(), ov.data()));
        return finish(outs, ov);
    }
    static std::vector<ArrayRef> cast(const std::vector<ArrayRef>& arr, DataType to) {
        // to and from Utf8 (Boolean, the integer types, Float32 / Float64): rdf_utf8_format / rdf_utf8_parse and their _float forms, the text staged through the host
        if (to == DataType::Utf8 || (!arr.empty() && arr[0]->dtype == DataType::Utf8))
            return Column::from_arrays(arr, Field{"cast", arr.empty() ? to : arr[0]->dtype, true}).cast_text(to).data().chunks();
        std::vector<rdf_array> a;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& x : arr) { a.push_back(x->view()); outs.push_back(Array::make_out(to, x->length, true, x->host)); ov.push_back(outs.back()->out_view(x->length)); }   // (a value the target type cannot hold becomes NULL: always a bitmap)
        check(rdf_cast(a.data(), (int64_t)a.size(), ov.data()));
        return finish(outs, ov);
    }
    // src/functions/scalar.rs:267-273: hour of day of a temporal column, given as its Int32 / Int64 storage + time unit
    static std::vector<ArrayRef> hour(const std::vector<ArrayRef>& arr, rdf_time_unit unit) {
        std::vector<rdf_array> a;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& x : arr) { a.push_back(x->view()); outs.push_back(Array::make_out(DataType::Int32, x->length, x->validity != nullptr, x->host)); ov.push_back(outs.back()->out_view(x->length)); }
        check(rdf_hour(a.data(), (int64_t)a.size(), (int32_t)unit, ov.data()));
        return finish(outs, ov);
    }
    // length / octet_length / locate / instr and the text predicates over Utf8 arrays (length, locate, ... are declared with
    // empty bodies, src/functions/scalar.rs:287-290): SQL / Spark semantics on the device (rdf_utf8_measure / rdf_utf8_predicate)
    // -> Int32 / Boolean arrays on the device, a NULL row gives NULL.  locate: the 1-based code-point position of the first
    // `substr` at or after position `pos`, 0 = none or pos < 1 (Python's s.find(sub, pos - 1) + 1); instr is pos = 1.
    static Column text_column(const std::vector<ArrayRef>& arr, const char* what) {
        for (auto& a : arr) if (a->dtype != DataType::Utf8) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": Utf8 arrays only");
        return Column::from_arrays(arr, Field{what, DataType::Utf8, true});
    }
    static std::vector<ArrayRef> length(const std::vector<ArrayRef>& arr) { return text_column(arr, "length").utf8_measure(RDF_UTF8_LENGTH).data().chunks(); }
    static std::vector<ArrayRef> octet_length(const std::vector<ArrayRef>& arr) { return text_column(arr, "octet_length").utf8_measure(RDF_UTF8_OCTET_LENGTH).data().chunks(); }
    static std::vector<ArrayRef> locate(const std::string& substr, const std::vector<ArrayRef>& arr, int64_t pos = 1) {
        return text_column(arr, "locate").utf8_measure(RDF_UTF8_LOCATE, substr, pos).data().chunks();
    }
    static std::vector<ArrayRef> instr(const std::vector<ArrayRef>& arr, const std::string& substr) { return locate(substr, arr, 1); }
    static std::vector<ArrayRef> starts_with(const std::vector<ArrayRef>& arr, const std::string& prefix) {
        return text_column(arr, "starts_with").utf8_predicate(RDF_UTF8_STARTS_WITH, prefix).data().chunks();
    }
    static std::vector<ArrayRef> ends_with(const std::vector<ArrayRef>& arr, const std::string& suffix) {
        return text_column(arr, "ends_with").utf8_predicate(RDF_UTF8_ENDS_WITH, suffix).data().chunks();
    }
    static std::vector<ArrayRef> contains(const std::vector<ArrayRef>& arr, const std::string& substr) {
        return text_column(arr, "contains").utf8_predicate(RDF_UTF8_CONTAINS, substr).data().chunks();
    }
    static std::vector<ArrayRef> like(const std::vector<ArrayRef>& arr, const std::string& pattern, int32_t escape = -1) {
        return text_column(arr, "like").utf8_predicate(RDF_UTF8_LIKE, pattern, escape).data().chunks();
    }
    // to_date(s, fmt) / to_timestamp / unix_timestamp / from_unix_time / date_format (src/functions/scalar.rs:459, 461, 473, 262, 209:
    // empty bodies): Spark 3's datetime patterns on the device (rdf_utf8_parse / rdf_utf8_format).  Parsing gives Int32 day
    // numbers / Int64 timestamps in `unit` (unix_timestamp: seconds), NULL where a row does not parse; formatting gives Utf8.
    static std::vector<ArrayRef> to_date(const std::vector<ArrayRef>& arr, const std::string& fmt) { return text_column(arr, "to_date").to_date(fmt).data().chunks(); }
    static std::vector<ArrayRef> to_timestamp(const std::vector<ArrayRef>& arr, rdf_time_unit unit, const std::string& fmt) {
        return text_column(arr, "to_timestamp").to_timestamp(unit, fmt).data().chunks();
    }
    static std::vector<ArrayRef> unix_timestamp(const std::vector<ArrayRef>& arr, const std::string& fmt) { return text_column(arr, "unix_timestamp").unix_timestamp(fmt).data().chunks(); }
    static std::vector<ArrayRef> from_unix_time(const std::vector<ArrayRef>& arr, const std::string& fmt) {
        return Column::utf8_format(arr, RDF_TEXT_TIMESTAMP, RDF_TIME_SECOND, &fmt, "from_unix_time").data().chunks();
    }
    static std::vector<ArrayRef> date_format(const std::vector<ArrayRef>& arr, rdf_time_unit unit, const std::string& fmt) {
        return Column::utf8_format(arr, RDF_TEXT_TIMESTAMP, (int32_t)unit, &fmt, "date_format").data().chunks();
    }
    // concat / concat_ws / lpad / rpad / repeat / reverse / substring_index over Utf8 arrays (declared with empty bodies in
    // src/functions/scalar.rs): Spark 3's semantics on the device (rdf_utf8_concat .. rdf_utf8_substring_index), Utf8 arrays
    // out.  A concat part is a chunk list or a std::string literal; all chunk lists of one call share one chunking.
    struct TextPart {
        std::vector<ArrayRef> arrays;
        std::string literal;
        bool is_literal;
        TextPart(std::vector<ArrayRef> a) : arrays(std::move(a)), is_literal(false) {}
        TextPart(std::string s) : literal(std::move(s)), is_literal(true) {}
        TextPart(const char* s) : literal(s), is_literal(true) {}
    };
    static std::vector<ArrayRef> concat_parts(const std::vector<TextPart>& parts, bool ws, const std::string& sep) {
        std::vector<Column> cols;
        cols.reserve(parts.size());
        for (auto& p : parts)
            if (!p.is_literal) cols.push_back(text_column(p.arrays, ws ? "concat_ws" : "concat"));
        std::vector<Column::Utf8Part> cp;
        size_t k = 0;
        for (auto& p : parts) {
            if (p.is_literal) cp.emplace_back(p.literal);
            else cp.emplace_back(cols[k++]);
        }
        return (ws ? Column::concat_ws(sep, cp) : Column::concat(cp)).data().chunks();
    }
    static std::vector<ArrayRef> concat(const std::vector<TextPart>& parts) { return concat_parts(parts, false, std::string()); }
    static std::vector<ArrayRef> concat_ws(const std::string& sep, const std::vector<TextPart>& parts) { return concat_parts(parts, true, sep); }
    static std::vector<ArrayRef> lpad(const std::vector<ArrayRef>& arr, int64_t len, const std::string& pad) { return text_column(arr, "lpad").lpad(len, pad).data().chunks(); }
    static std::vector<ArrayRef> rpad(const std::vector<ArrayRef>& arr, int64_t len, const std::string& pad) { return text_column(arr, "rpad").rpad(len, pad).data().chunks(); }
    static std::vector<ArrayRef> repeat(const std::vector<ArrayRef>& arr, int64_t times) { return text_column(arr, "repeat").repeat(times).data().chunks(); }
    static std::vector<ArrayRef> reverse(const std::vector<ArrayRef>& arr) { return text_column(arr, "reverse").reverse().data().chunks(); }
    static std::vector<ArrayRef> substring_index(const std::vector<ArrayRef>& arr, const std::string& delim, int64_t count) {
        return text_column(arr, "substring_index").substring_index(delim, count).data().chunks();
    }
    // replace / translate / initcap / split over Utf8 arrays (initcap, translate and split are declared with empty bodies in
    // src/functions/scalar.rs): Spark 3's semantics on the device (rdf_utf8_replace .. rdf_utf8_split).  split takes a LITERAL
    // delimiter and returns ONE ListArray over all chunks whose child is a Utf8 array, so explode() above takes it as it is.
    static std::vector<ArrayRef> replace(const std::vector<ArrayRef>& arr, const std::string& search, const std::string& replacement) {
        return text_column(arr, "replace").replace(search, replacement).data().chunks();
    }
    static std::vector<ArrayRef> translate(const std::vector<ArrayRef>& arr, const std::string& matching, const std::string& replace) {
        return text_column(arr, "translate").translate(matching, replace).data().chunks();
    }
    static std::vector<ArrayRef> initcap(const std::vector<ArrayRef>& arr) { return text_column(arr, "initcap").initcap().data().chunks(); }
    static inline ListArray split(const std::vector<ArrayRef>& arr, const std::string& delim, int64_t limit = -1);
    // rlike / regexp_count / regexp_extract / regexp_replace / split_regexp over Utf8 arrays (regexp_extract and regexp_replace are
    // declared with empty bodies in src/functions/scalar.rs): java.util.regex's leftmost-first matching on the device
    // (rdf_utf8_regexp_match .. rdf_utf8_regexp_split) -> Boolean / Int32 / Utf8 arrays, and ONE ListArray as split returns it.
    static std::vector<ArrayRef> rlike(const std::vector<ArrayRef>& arr, const std::string& pattern) { return text_column(arr, "rlike").rlike(pattern).data().chunks(); }
    static std::vector<ArrayRef> regexp_count(const std::vector<ArrayRef>& arr, const std::string& pattern) {
        return text_column(arr, "regexp_count").regexp_count(pattern).data().chunks();
    }
    static std::vector<ArrayRef> regexp_extract(const std::vector<ArrayRef>& arr, const std::string& pattern, int32_t group = 0) {
        return text_column(arr, "regexp_extract").regexp_extract(pattern, group).data().chunks();
    }
    static std::vector<ArrayRef> regexp_replace(const std::vector<ArrayRef>& arr, const std::string& pattern, const std::string& replacement) {
        return text_column(arr, "regexp_replace").regexp_replace(pattern, replacement).data().chunks();
    }
    static inline ListArray split_regexp(const std::vector<ArrayRef>& arr, const std::string& pattern, int64_t limit = -1);
    // hash / xxhash64 / crc32 / md5 / sha1 / sha2 (declared with empty bodies, src/functions/scalar.rs:205, :265, :338, :389, :390):
    // Spark 3's semantics on the device (rdf_hash_columns / rdf_utf8_crc32 / rdf_utf8_digest).  hash and xxhash64 take the columns
    // as chunk lists of one chunking, numeric, Boolean or Utf8, and return Int32 / Int64 arrays that are never NULL; the digests
    // take Utf8 arrays and return Utf8 arrays (lowercase hex), crc32 Int64 arrays; a NULL row gives NULL.
    static std::vector<ArrayRef> hash_kind(int32_t kind, const std::vector<std::vector<ArrayRef>>& cols, int64_t seed) {
        std::vector<Column> cs;
        cs.reserve(cols.size());
        for (auto& arr : cols) {
            if (arr.empty()) throw DataFrameError(DataFrameError::ComputeError, "hash: a column without chunks");
            cs.push_back(Column::from_arrays(arr, Field{"hash", arr[0]->dtype, true}));
        }
        std::vector<const Column*> ptrs;
        for (auto& c : cs) ptrs.push_back(&c);
        return Column::hash_columns(kind, ptrs, seed).data().chunks();
    }
    static std::vector<ArrayRef> hash(const std::vector<std::vector<ArrayRef>>& cols, int64_t seed = 42) { return hash_kind(RDF_HASH_MURMUR3_32, cols, seed); }
    static std::vector<ArrayRef> xxhash64(const std::vector<std::vector<ArrayRef>>& cols, int64_t seed = 42) { return hash_kind(RDF_HASH_XXHASH64, cols, seed); }
    static std::vector<ArrayRef> crc32(const std::vector<ArrayRef>& arr) { return text_column(arr, "crc32").crc32().data().chunks(); }
    static std::vector<ArrayRef> md5(const std::vector<ArrayRef>& arr) { return text_column(arr, "md5").md5().data().chunks(); }
    static std::vector<ArrayRef> sha1(const std::vector<ArrayRef>& arr) { return text_column(arr, "sha1").sha1().data().chunks(); }
    static std::vector<ArrayRef> sha2(const std::vector<ArrayRef>& arr, int32_t bits) { return text_column(arr, "sha2").sha2(bits).data().chunks(); }
    // The calendar functions src/functions/scalar.rs declares with empty bodies (year .. date_diff): Spark 3's semantics as
    // written down at rdf_datetime_fields in rdf_mi355x.h.  Like hour, a temporal column is its Int32 / Int64 storage + time unit.
    // datetime_fields reads the column ONCE for up to 8 fields and returns one chunk list per field, in the order asked for.
    static std::vector<std::vector<ArrayRef>> datetime_fields(const std::vector<ArrayRef>& arr, rdf_time_unit unit, const std::vector<rdf_datetime_field>& fields) {
        std::vector<rdf_array> a;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        std::vector<int32_t> codes(fields.begin(), fields.end());
        for (auto& x : arr) a.push_back(x->view());
        for (size_t f = 0; f < fields.size(); ++f)
            for (auto& x : arr) { outs.push_back(Array::make_out(DataType::Int32, x->length, x->validity != nullptr, x->host)); ov.push_back(outs.back()->out_view(x->length)); }
        check(rdf_datetime_fields(a.data(), (int64_t)a.size(), (int32_t)unit, codes.data(), (int32_t)codes.size(), ov.data()));
        const std::vector<ArrayRef> flat = finish(outs, ov);
        std::vector<std::vector<ArrayRef>> per_field(fields.size());
        for (size_t f = 0; f < fields.size(); ++f) per_field[f].assign(flat.begin() + f * arr.size(), flat.begin() + (f + 1) * arr.size());
        return per_field;
    }
    static std::vector<ArrayRef> datetime_field(const std::vector<ArrayRef>& arr, rdf_time_unit unit, rdf_datetime_field field) { return datetime_fields(arr, unit, {field})[0]; }
    static std::vector<ArrayRef> year(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_YEAR); }
    static std::vector<ArrayRef> quarter(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_QUARTER); }
    static std::vector<ArrayRef> month(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_MONTH); }
    static std::vector<ArrayRef> day_of_month(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_DAY_OF_MONTH); }
    static std::vector<ArrayRef> day_of_week(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_DAY_OF_WEEK); }   // 1 = Sunday
    static std::vector<ArrayRef> day_of_year(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_DAY_OF_YEAR); }
    static std::vector<ArrayRef> week_of_year(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_WEEK_OF_YEAR); }   // ISO-8601
    static std::vector<ArrayRef> minute(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_MINUTE); }
    static std::vector<ArrayRef> second(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_SECOND); }
    static std::vector<ArrayRef> to_date(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return datetime_field(a, unit, RDF_DT_DATE); }   // Int32 day numbers
    // date_trunc(level, ts): same storage and unit out; trunc(date, level) is date_trunc over Int32 day numbers
    static std::vector<ArrayRef> date_trunc(const std::vector<ArrayRef>& arr, rdf_time_unit unit, rdf_trunc_level level) {
        std::vector<rdf_array> a;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& x : arr) { a.push_back(x->view()); outs.push_back(Array::make_out(x->dtype, x->length, x->validity != nullptr, x->host)); ov.push_back(outs.back()->out_view(x->length)); }
        check(rdf_datetime_trunc(a.data(), (int64_t)a.size(), (int32_t)unit, (int32_t)level, ov.data()));
        return finish(outs, ov);
    }
    static std::vector<ArrayRef> trunc(const std::vector<ArrayRef>& dates, rdf_trunc_level level) { return date_trunc(dates, RDF_TIME_DAY, level); }
    // date_add / date_sub / add_months / last_day / next_day -> Int32 day numbers; the amount is one number or an Int32 column
    static std::vector<ArrayRef> date_shift(const std::vector<ArrayRef>& arr, rdf_time_unit unit, rdf_date_shift_op op, const std::vector<ArrayRef>* amounts, int32_t amount) {
        if (amounts && amounts->size() != arr.size()) throw DataFrameError(DataFrameError::ComputeError, "chunk lists differ in length");
        std::vector<rdf_array> a, k;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t i = 0; i < arr.size(); ++i) {
            a.push_back(arr[i]->view());
            if (amounts) k.push_back((*amounts)[i]->view());
            const bool nullable = arr[i]->validity || (amounts && ((*amounts)[i]->validity || op == RDF_SHIFT_NEXT_DAY));   // (a per-row weekday outside 1..7 is a NULL row)
            outs.push_back(Array::make_out(DataType::Int32, arr[i]->length, nullable, arr[i]->host));
            ov.push_back(outs.back()->out_view(arr[i]->length));
        }
        check(::rdf_date_shift(a.data(), (int64_t)a.size(), (int32_t)unit, (int32_t)op, amounts ? k.data() : nullptr, amount, ov.data()));
        return finish(outs, ov);
    }
    static std::vector<ArrayRef> date_add(const std::vector<ArrayRef>& a, rdf_time_unit unit, int32_t days) { return date_shift(a, unit, RDF_SHIFT_DAYS, nullptr, days); }
    static std::vector<ArrayRef> date_add(const std::vector<ArrayRef>& a, rdf_time_unit unit, const std::vector<ArrayRef>& days) { return date_shift(a, unit, RDF_SHIFT_DAYS, &days, 0); }
    static std::vector<ArrayRef> date_sub(const std::vector<ArrayRef>& a, rdf_time_unit unit, int32_t days) { return date_shift(a, unit, RDF_SHIFT_DAYS, nullptr, (int32_t)(0u - (uint32_t)days)); }
    static std::vector<ArrayRef> date_sub(const std::vector<ArrayRef>& a, rdf_time_unit unit, const std::vector<ArrayRef>& days) {
        return binary(RDF_OP_SUB, to_date(a, unit), days);   // day number - days: Int32, wrapping, validity ANDed
    }
    static std::vector<ArrayRef> add_months(const std::vector<ArrayRef>& a, rdf_time_unit unit, int32_t months) { return date_shift(a, unit, RDF_SHIFT_MONTHS, nullptr, months); }
    static std::vector<ArrayRef> add_months(const std::vector<ArrayRef>& a, rdf_time_unit unit, const std::vector<ArrayRef>& months) { return date_shift(a, unit, RDF_SHIFT_MONTHS, &months, 0); }
    static std::vector<ArrayRef> last_day(const std::vector<ArrayRef>& a, rdf_time_unit unit) { return date_shift(a, unit, RDF_SHIFT_LAST_DAY, nullptr, 0); }
    static std::vector<ArrayRef> next_day(const std::vector<ArrayRef>& a, rdf_time_unit unit, int32_t weekday) { return date_shift(a, unit, RDF_SHIFT_NEXT_DAY, nullptr, weekday); }   // 1 = Sunday .. 7
    static std::vector<ArrayRef> next_day(const std::vector<ArrayRef>& a, rdf_time_unit unit, const std::vector<ArrayRef>& weekdays) { return date_shift(a, unit, RDF_SHIFT_NEXT_DAY, &weekdays, 0); }
    // date_diff(end, start) = day(end) - day(start), each column with its own storage and unit
    static std::vector<ArrayRef> date_diff(const std::vector<ArrayRef>& end, rdf_time_unit end_unit, const std::vector<ArrayRef>& start, rdf_time_unit start_unit) {
        if (end.size() != start.size()) throw DataFrameError(DataFrameError::ComputeError, "chunk lists differ in length");
        std::vector<rdf_array> a, b;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t i = 0; i < end.size(); ++i) {
            a.push_back(end[i]->view()); b.push_back(start[i]->view());
            outs.push_back(Array::make_out(DataType::Int32, end[i]->length, end[i]->validity || start[i]->validity, end[i]->host));
            ov.push_back(outs.back()->out_view(end[i]->length));
        }
        check(rdf_date_diff(a.data(), (int32_t)end_unit, b.data(), (int32_t)start_unit, (int64_t)a.size(), ov.data()));
        return finish(outs, ov);
    }
    // src/functions/scalar.rs:16-103
    static std::vector<ArrayRef> add(const std::vector<ArrayRef>& l, const std::vector<ArrayRef>& r) { return binary(RDF_OP_ADD, l, r); }
    static std::vector<ArrayRef> subtract(const std::vector<ArrayRef>& l, const std::vector<ArrayRef>& r) { return binary(RDF_OP_SUB, l, r); }
    static std::vector<ArrayRef> multiply(const std::vector<ArrayRef>& l, const std::vector<ArrayRef>& r) { return binary(RDF_OP_MUL, l, r); }
    static std::vector<ArrayRef> divide(const std::vector<ArrayRef>& l, const std::vector<ArrayRef>& r) { return binary(RDF_OP_DIV, l, r); }
    // :106-452
    static std::vector<ArrayRef> abs(const std::vector<ArrayRef>& a) { return unary(RDF_OP_ABS, a); }
    static std::vector<ArrayRef> sin(const std::vector<ArrayRef>& a) { return unary(RDF_OP_SIN, a); }
    static std::vector<ArrayRef> cos(const std::vector<ArrayRef>& a) { return unary(RDF_OP_COS, a); }
    static std::vector<ArrayRef> tan(const std::vector<ArrayRef>& a) { return unary(RDF_OP_TAN, a); }
    static std::vector<ArrayRef> cot(const std::vector<ArrayRef>& a) { return unary(RDF_OP_COT, a); }
    static std::vector<ArrayRef> sec(const std::vector<ArrayRef>& a) { return unary(RDF_OP_SEC, a); }
    static std::vector<ArrayRef> csc(const std::vector<ArrayRef>& a) { return unary(RDF_OP_CSC, a); }
    static std::vector<ArrayRef> acos(const std::vector<ArrayRef>& a) { return unary(RDF_OP_ACOS, a); }

    // coalesce / greatest / least / nanv1 / when, which src/functions/scalar.rs declares with empty bodies, and is_null /
    // is_not_null / isnan as masks: Spark 3's semantics as written down at rdf_coalesce in rdf_mi355x.h.  A Value is a column's
    // chunks or a Scalar literal (Scalar() is the NULL literal), converted to the dtype of the call's first column.
    struct Value {
        std::vector<ArrayRef> column;
        Scalar literal;
        bool is_column;
        Value(std::vector<ArrayRef> c) : column(std::move(c)), is_column(true) {}
        Value(Scalar s) : literal(std::move(s)), is_column(false) {}
    };
    static std::vector<ArrayRef> coalesce(const std::vector<Value>& parts) { return select_call(0, parts, {}, nullptr, false); }
    static std::vector<ArrayRef> greatest(const std::vector<Value>& parts) { return select_call(2, parts, {}, nullptr, true); }
    static std::vector<ArrayRef> least(const std::vector<Value>& parts) { return select_call(2, parts, {}, nullptr, false); }
    static std::vector<ArrayRef> nanvl(const Value& a, const Value& b) { return select_call(3, {a, b}, {}, nullptr, false); }
    // when(c0, v0).when(c1, v1).otherwise(v): the first condition that is valid AND true chooses; end(): no otherwise, NULL
    struct When {
        std::vector<std::vector<ArrayRef>> conds;
        std::vector<Value> values;
        When& when(std::vector<ArrayRef> cond, Value value) { conds.push_back(std::move(cond)); values.push_back(std::move(value)); return *this; }
        std::vector<ArrayRef> otherwise(const Value& value) const { return select_call(1, values, conds, &value, false); }
        std::vector<ArrayRef> end() const { return select_call(1, values, conds, nullptr, false); }
    };
    static When when(std::vector<ArrayRef> cond, Value value) { When w; w.when(std::move(cond), std::move(value)); return w; }
    static std::vector<ArrayRef> null_test(rdf_null_test_op op, const std::vector<ArrayRef>& arr) {
        if (!arr.empty() && arr[0]->dtype == DataType::Utf8) {   // a text column: the rows' bitmap
            const Column c = text_column(arr, "is_null");
            return (op == RDF_IS_NULL ? c.is_null() : op == RDF_IS_NOT_NULL ? c.is_not_null() : c.is_nan()).data().chunks();
        }
        std::vector<rdf_array> a;
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (auto& x : arr) { a.push_back(x->view()); outs.push_back(Array::make_out(DataType::Boolean, x->length, false, x->host)); ov.push_back(outs.back()->out_view(x->length)); }
        check(rdf_null_test((int32_t)op, a.data(), (int64_t)a.size(), ov.data()));
        return finish(outs, ov);
    }
    static std::vector<ArrayRef> is_null(const std::vector<ArrayRef>& a) { return null_test(RDF_IS_NULL, a); }
    static std::vector<ArrayRef> is_not_null(const std::vector<ArrayRef>& a) { return null_test(RDF_IS_NOT_NULL, a); }
    static std::vector<ArrayRef> is_nan(const std::vector<ArrayRef>& a) { return null_test(RDF_IS_NAN, a); }

  private:
    static uint64_t literal_bits(const Scalar& s, DataType dt) {
        const bool fl = s.kind == Scalar::Float32 || s.kind == Scalar::Float64;
        if (!fl && s.kind != Scalar::Int32 && s.kind != Scalar::Int64) throw DataFrameError(DataFrameError::ComputeError, "a literal of these functions is a number or NULL");
        uint64_t bits = 0;
        if (dt == DataType::Float64) { const double d = fl ? s.f : (double)s.i; std::memcpy(&bits, &d, 8); }
        else if (dt == DataType::Float32) { const float f = fl ? (float)s.f : (float)s.i; std::memcpy(&bits, &f, 4); }
        else bits = (uint64_t)(fl ? (int64_t)s.f : s.i);            // (the library keeps the low bytes of the call's dtype)
        return bits;
    }
    // coalesce / when over Utf8 chunk lists: columns staged as concat stages them, Scalar::String literals, Scalar() = NULL
    static std::vector<ArrayRef> text_select_call(int kind, const std::vector<const Value*>& slots, size_t nvalues, const std::vector<std::vector<ArrayRef>>& conds, bool has_otherwise) {
        if (kind > 1) throw DataFrameError(DataFrameError::ComputeError, "greatest / least / nanvl do not support type Utf8");
        const char* what = kind ? "when" : "coalesce";
        std::vector<Column> cols, ccols;
        cols.reserve(slots.size());
        ccols.reserve(conds.size());
        for (auto* v : slots)
            if (v->is_column) cols.push_back(text_column(v->column, what));
        for (auto& c : conds) {
            for (auto& x : c)
                if (x->dtype != DataType::Boolean) throw DataFrameError(DataFrameError::ComputeError, "when: a condition is a Boolean column");
            ccols.push_back(Column::from_arrays(c, Field{"when", DataType::Boolean, true}));
        }
        std::vector<Column::TextValue> tv;
        size_t k = 0;
        for (auto* v : slots) {
            if (v->is_column) tv.emplace_back(cols[k++]);
            else if (v->literal.kind == Scalar::Null) tv.push_back(Column::TextValue::null_literal());
            else if (v->literal.kind == Scalar::String) tv.emplace_back(v->literal.s);
            else throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": a literal for a Utf8 column is a Scalar::String or NULL");
        }
        std::vector<const Column*> cp;
        for (auto& c : ccols) cp.push_back(&c);
        const std::vector<Column::TextValue> values(tv.begin(), tv.begin() + (std::ptrdiff_t)nvalues);
        return Column::text_select(cp, values, has_otherwise ? &tv[nvalues] : nullptr, what).data().chunks();
    }
    // kind: 0 coalesce, 1 case_when (values + conds + otherwise), 2 extremum, 3 nanvl
    static std::vector<ArrayRef> select_call(int kind, const std::vector<Value>& values, const std::vector<std::vector<ArrayRef>>& conds, const Value* otherwise, bool greatest) {
        std::vector<const Value*> slots;
        for (auto& v : values) slots.push_back(&v);
        if (otherwise) slots.push_back(otherwise);
        const std::vector<ArrayRef>* first = nullptr;
        for (auto* v : slots) if (v->is_column && !first) first = &v->column;
        if (!first) throw DataFrameError(DataFrameError::ComputeError, "at least one part must be a column");
        const size_t n = first->size();
        const DataType dt = n ? (*first)[0]->dtype : DataType::Float64;
        if (kind == 1 && conds.size() != values.size()) throw DataFrameError(DataFrameError::ComputeError, "one value per condition");
        if (dt == DataType::Utf8) return text_select_call(kind, slots, values.size(), conds, otherwise != nullptr);
        std::vector<std::vector<rdf_array>> views(slots.size()), cviews(conds.size());
        std::vector<rdf_value_part> parts(slots.size());
        for (size_t k = 0; k < slots.size(); ++k) {
            parts[k] = rdf_value_part{nullptr, 0, 0};
            if (slots[k]->is_column) {
                if (slots[k]->column.size() != n) throw DataFrameError(DataFrameError::ComputeError, "chunk lists differ in length");
                for (auto& x : slots[k]->column) views[k].push_back(x->view());
                parts[k].column = views[k].data();
            } else if (slots[k]->literal.kind == Scalar::Null) parts[k].literal_is_null = 1;
            else parts[k].literal_bits = literal_bits(slots[k]->literal, dt);
        }
        std::vector<const rdf_array*> cptr;
        for (size_t k = 0; k < conds.size(); ++k) {
            if (conds[k].size() != n) throw DataFrameError(DataFrameError::ComputeError, "chunk lists differ in length");
            for (auto& x : conds[k]) cviews[k].push_back(x->view());
            cptr.push_back(cviews[k].data());
        }
        std::vector<std::shared_ptr<Array>> outs;
        std::vector<rdf_out> ov;
        for (size_t c = 0; c < n; ++c) {
            bool any_nullable = kind == 1 && !otherwise, all_nullable = true;
            for (auto* v : slots) {
                const bool nullable = v->is_column ? v->column[c]->validity != nullptr : v->literal.kind == Scalar::Null;
                any_nullable = any_nullable || nullable;
                all_nullable = all_nullable && nullable;
            }
            const bool with_validity = (kind == 0 || kind == 2) ? all_nullable : any_nullable;
            outs.push_back(Array::make_out(dt, (*first)[c]->length, with_validity, (*first)[c]->host));
            ov.push_back(outs.back()->out_view((*first)[c]->length));
        }
        const size_t nv = values.size();
        switch (kind) {
            case 0: check(rdf_coalesce(parts.data(), (int32_t)nv, (int64_t)n, ov.data())); break;
            case 1: check(rdf_case_when(cptr.data(), parts.data(), (int32_t)nv, otherwise ? &parts[nv] : nullptr, (int64_t)n, ov.data())); break;
            case 2: check(rdf_extremum(greatest ? 1 : 0, parts.data(), (int32_t)nv, (int64_t)n, ov.data())); break;
            default: check(rdf_nanvl(&parts[0], &parts[1], (int64_t)n, ov.data())); break;
        }
        return finish(outs, ov);
    }
    static inline DataFrame explode_rows(const DataFrame& frame, const ListArray& list, const std::string* pos_name, const std::string& name, bool outer);
    static std::vector<ArrayRef> finish(std::vector<std::shared_ptr<Array>>& outs, std::vector<rdf_out>& ov) {
        std::vector<ArrayRef> res;
        for (size_t i = 0; i < outs.size(); ++i) { outs[i]->length = ov[i].length; outs[i]->null_count = ov[i].null_count; res.push_back(outs[i]); }
        return res;
    }
};

inline Column Column::coalesce(const Column& other) const {
    if (data_type() == DataType::Utf8) return text_select({}, {TextValue(*this), TextValue(other)}, nullptr, field_.name);
    return Column::from_arrays(ScalarFunctions::coalesce({data_.chunks(), other.data().chunks()}), field_);
}
inline Column Column::fill_null(const Scalar& value) const {
    if (data_type() == DataType::Utf8) {
        if (value.kind != Scalar::String) throw DataFrameError(DataFrameError::ComputeError, "fill_null: a Utf8 column takes a Scalar::String");
        return text_select({}, {TextValue(*this), TextValue(value.s)}, nullptr, field_.name);
    }
    return Column::from_arrays(ScalarFunctions::coalesce({data_.chunks(), value}), field_);
}
inline Column Column::greatest(const Column& other) const { return Column::from_arrays(ScalarFunctions::greatest({data_.chunks(), other.data().chunks()}), field_); }
inline Column Column::least(const Column& other) const { return Column::from_arrays(ScalarFunctions::least({data_.chunks(), other.data().chunks()}), field_); }
inline Column Column::nanvl(const Column& other) const { return Column::from_arrays(ScalarFunctions::nanvl(data_.chunks(), other.data().chunks()), field_); }
inline Column Column::text_null_test(int32_t op) const {   // the rows' bitmap of the staged offsets array; values are never read
    if (op == RDF_IS_NAN) throw DataFrameError(DataFrameError::ComputeError, "is_nan does not support type Utf8");
    const TextChunks tc = text_chunks("is_null");
    std::vector<rdf_array> a;
    for (auto& u : tc.txt) a.push_back(rdf_array{nullptr, u.offsets.validity, u.offsets.offset, u.offsets.length - 1, -1, RDF_I32, RDF_MEM_HOST});
    Column r = text_result(DataType::Boolean, tc, std::vector<bool>(a.size(), false), field_.name, false, [&](rdf_out* outs) {
        check(rdf_null_test(op, a.data(), (int64_t)a.size(), outs));
    });
    return Column(r.data(), Field{field_.name, DataType::Boolean, false});
}
inline Column Column::is_null() const {
    if (data_type() == DataType::Utf8) return text_null_test(RDF_IS_NULL);
    return Column::from_arrays(ScalarFunctions::is_null(data_.chunks()), Field{field_.name, DataType::Boolean, false});
}
inline Column Column::is_in(const Column& set) const {
    return DataFrame::from_columns({*this}).member_mask(DataFrame::from_columns({set}), {{name(), set.name()}}, RDF_MEMBER_IS_IN, name());
}
inline Column Column::is_not_null() const {
    if (data_type() == DataType::Utf8) return text_null_test(RDF_IS_NOT_NULL);
    return Column::from_arrays(ScalarFunctions::is_not_null(data_.chunks()), Field{field_.name, DataType::Boolean, false});
}
inline Column Column::is_nan() const {
    if (data_type() == DataType::Utf8) return text_null_test(RDF_IS_NAN);
    return Column::from_arrays(ScalarFunctions::is_nan(data_.chunks()), Field{field_.name, DataType::Boolean, false});
}

struct AggregateFunctions {  // src/functions/aggregate.rs:12-93
    template <class T> static std::optional<T> call(rdf_status (*fn)(const rdf_array*, int64_t, void*, int32_t*), const ChunkedArray& c) {
        const auto v = c.views();
        T out{}; int32_t some = 0;
        check(fn(v.data(), (int64_t)v.size(), &out, &some));
        return some ? std::optional<T>(out) : std::nullopt;
    }
    template <class T> static std::optional<T> sum(const ChunkedArray& c) { return call<T>(rdf_sum, c); }
    template <class T> static std::optional<T> min(const ChunkedArray& c) { return call<T>(rdf_min, c); }
    template <class T> static std::optional<T> max(const ChunkedArray& c) { return call<T>(rdf_max, c); }
    static std::optional<int64_t> count(const ChunkedArray& c) {
        const auto v = c.views(); int64_t out = 0; int32_t some = 0;
        check(rdf_count(v.data(), (int64_t)v.size(), &out, &some));
        return some ? std::optional<int64_t>(out) : std::nullopt;
    }
    static std::optional<double> avg(const ChunkedArray& c) {
        const auto v = c.views(); double out = 0; int32_t some = 0;
        check(rdf_avg(v.data(), (int64_t)v.size(), &out, &some));
        return some ? std::optional<double>(out) : std::nullopt;
    }

    // variance / stddev / skewness / kurtosis (:94-102, declared with empty bodies and a TODO for "population and sample")
    // and ScalarFunctions::corr (src/functions/scalar.rs:184) with Spark's definitions: ONE pass over the column gives a
    // state, every statistic is read off it, and states of shards merge.  `mask` (a Boolean column chunked like the data)
    // is Column::filter's condition: filter -> variance without the compacted copy.
    struct Moments {
        rdf_moments_state state{};
        int64_t count() const { return state.count; }
        Moments& merge(const Moments& other) { check(rdf_moments_merge(&state, &other.state)); return *this; }
        std::optional<double> stat(rdf_stat which) const {
            double out = 0; int32_t some = 0;
            check(rdf_moments_stat(&state, (int32_t)which, &out, &some));
            return some ? std::optional<double>(out) : std::nullopt;
        }
    };
    struct Comoments {
        rdf_comoments_state state{};
        int64_t count() const { return state.count; }
        Comoments& merge(const Comoments& other) { check(rdf_comoments_merge(&state, &other.state)); return *this; }
        std::optional<double> stat(rdf_costat which) const {
            double out = 0; int32_t some = 0;
            check(rdf_comoments_stat(&state, (int32_t)which, &out, &some));
            return some ? std::optional<double>(out) : std::nullopt;
        }
    };
    static Moments moments(const ChunkedArray& c, const ChunkedArray* mask = nullptr) {
        const auto v = c.views();
        const auto m = mask_views(mask, v.size());
        Moments r;
        check(rdf_moments(v.data(), mask ? m.data() : nullptr, (int64_t)v.size(), &r.state));
        return r;
    }
    static Comoments comoments(const ChunkedArray& x, const ChunkedArray& y, const ChunkedArray* mask = nullptr) {
        const auto vx = x.views(), vy = y.views();
        if (vx.size() != vy.size()) throw DataFrameError(DataFrameError::ComputeError, "comoments: chunk counts differ");
        const auto m = mask_views(mask, vx.size());
        Comoments r;
        check(rdf_comoments(vx.data(), vy.data(), mask ? m.data() : nullptr, (int64_t)vx.size(), &r.state));
        return r;
    }
    // the sample forms, as Spark's `variance` / `stddev`
    static std::optional<double> variance(const ChunkedArray& c, const ChunkedArray* mask = nullptr) { return moments(c, mask).stat(RDF_STAT_VAR_SAMP); }
    static std::optional<double> stddev(const ChunkedArray& c, const ChunkedArray* mask = nullptr) { return moments(c, mask).stat(RDF_STAT_STDDEV_SAMP); }
    static std::optional<double> var_pop(const ChunkedArray& c, const ChunkedArray* mask = nullptr) { return moments(c, mask).stat(RDF_STAT_VAR_POP); }
    static std::optional<double> stddev_pop(const ChunkedArray& c, const ChunkedArray* mask = nullptr) { return moments(c, mask).stat(RDF_STAT_STDDEV_POP); }
    static std::optional<double> skewness(const ChunkedArray& c, const ChunkedArray* mask = nullptr) { return moments(c, mask).stat(RDF_STAT_SKEWNESS); }
    static std::optional<double> kurtosis(const ChunkedArray& c, const ChunkedArray* mask = nullptr) { return moments(c, mask).stat(RDF_STAT_KURTOSIS); }
    static std::optional<double> corr(const ChunkedArray& x, const ChunkedArray& y, const ChunkedArray* mask = nullptr) { return comoments(x, y, mask).stat(RDF_COSTAT_CORR); }
    static std::optional<double> covar_pop(const ChunkedArray& x, const ChunkedArray& y, const ChunkedArray* mask = nullptr) { return comoments(x, y, mask).stat(RDF_COSTAT_COVAR_POP); }
    static std::optional<double> covar_samp(const ChunkedArray& x, const ChunkedArray& y, const ChunkedArray* mask = nullptr) { return comoments(x, y, mask).stat(RDF_COSTAT_COVAR_SAMP); }

    // count_distinct / sum_distinct / first / last (:66-93, declared with empty bodies) of a whole column, numeric or Utf8:
    // rdf_groupby_sorted with no grouping columns — distinctness as Column::uniques (floats canonical, Utf8 by bytes), NULL
    // rows never counted or summed.  An empty column gives 0 / 0 / none / none.
    //   count_distinct  keeps the hash route of rdf_uniques / rdf_utf8_uniques (count-only calls) for the dtypes those take
    //   sum_distinct<T> T = double for a float column, int64_t / uint64_t (wrapping) for an integer one; Utf8 is refused
    //   first / last    the row as a ONE-row column typed like the input (its row is NULL where the column's is), or, with
    //                   ignore_nulls, the first / last row that is not NULL; none for an empty column or one without such a row
    static int64_t count_distinct(const Column& c) {
        int64_t count = 0;
        const DataType dt = c.data_type();
        if (c.num_rows() == 0) return 0;
        if (dt == DataType::Int64 || dt == DataType::UInt64 || dt == DataType::Float64) {
            const auto v = c.data().views();
            check(rdf_uniques(v.data(), (int64_t)v.size(), nullptr, &count));
            return count;
        }
        const std::string name = c.name();
        const DataFrame f = DataFrame::from_columns({c});
        if (dt == DataType::Utf8) {
            // rdf_utf8_uniques has no count-only form of its own, so this is its SIZING call: an offsets buffer of one entry
            // and no data buffer can hold no distinct string, the call sets `count`, writes nothing and answers
            // RDF_MEMORY_ERROR — the one status that is not an error here; every other one is raised.
            // host = true whatever the frame holds: the mirror keeps a Utf8 column's strings on the host, and `host` only
            // says whether sort_keys copies them to the device to match numeric columns in the same call.  This call has no
            // numeric column to match and its two outputs are host memory, so the strings are handed over where they are.
            const DataFrame::SortKeys sk = f.sort_keys({DataFrame::SortCriteria{name, false, false}}, true);
            int32_t one = 0;
            rdf_out oo{&one, nullptr, 1, 0, 0, RDF_I32, RDF_MEM_HOST}, od{nullptr, nullptr, 0, 0, 0, RDF_U8, RDF_MEM_HOST};
            const rdf_status st = rdf_utf8_uniques(sk.txt[0].data(), (int64_t)sk.txt[0].size(), &oo, &od, &count);
            if (st != RDF_MEMORY_ERROR) check(st);
            return count;
        }
        const DataFrame::SortedGroups g = f.sorted_groups({}, &name, {rdf_group_call{RDF_GRP_COUNT_DISTINCT, 0}});
        return g.groups ? g.outs[0]->values_to_host<int64_t>()[0] : 0;
    }
    template <class T> static T sum_distinct(const Column& c) {
        static_assert(std::is_same<T, double>::value || std::is_same<T, int64_t>::value || std::is_same<T, uint64_t>::value, "double, int64_t or uint64_t");
        const DataType dt = c.data_type();
        if (!(is_integer(dt) || is_float(dt))) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column must be numeric");
        if (is_float(dt) != std::is_same<T, double>::value) throw DataFrameError(DataFrameError::ComputeError, "sum_distinct: double for a float column, a 64-bit integer otherwise");
        if (c.num_rows() == 0) return T(0);
        const std::string name = c.name();
        const DataFrame::SortedGroups g = DataFrame::from_columns({c}).sorted_groups({}, &name, {rdf_group_call{RDF_GRP_SUM_DISTINCT, 0}});
        if (!g.groups) return T(0);
        if (is_float(dt)) return (T)g.outs[0]->values_to_host<double>()[0];
        return (T)g.outs[0]->values_to_host<int64_t>()[0];
    }
    static std::optional<Column> first(const Column& c, bool ignore_nulls = false) { return first_or_last(c, RDF_GRP_FIRST, ignore_nulls); }
    static std::optional<Column> last(const Column& c, bool ignore_nulls = false) { return first_or_last(c, RDF_GRP_LAST, ignore_nulls); }

    // percentile / median / percentile_disc of a whole column over its non-NULL rows (Spark's aggregates of those names;
    // aggregate.rs stops before them): rdf_groupby_percentile with no grouping columns, which answers a numeric column by a
    // radix select instead of a sort.  p outside [0, 1] is refused.
    //   percentile(c, p)       Spark 3's `percentile`: pos = (m - 1) * p over the m sorted values, linear between the values at
    //                          floor(pos) and ceil(pos); numeric columns only.  none for an empty or all-NULL column
    //   percentiles(c, {p..})  up to 8 of them from one call, in the order given
    //   median(c)              percentile(c, 0.5)
    //   percentile_disc(c, p)  SQL's percentile_disc: the row holding the value at sorted position max(0, ceil(p * m) - 1), as
    //                          a ONE-row column typed like the input (numeric or Utf8), or none
    static std::vector<std::optional<double>> percentiles(const Column& c, const std::vector<double>& ps) {
        const DataType dt = c.data_type();
        if (!(is_integer(dt) || is_float(dt))) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column must be numeric");
        if (ps.size() > RDF_PERCENTILE_MAX_CALLS) throw DataFrameError(DataFrameError::ComputeError, "percentiles: at most " + std::to_string(RDF_PERCENTILE_MAX_CALLS) + " per call");
        std::vector<rdf_percentile_call> calls;
        for (double p : ps) {
            if (!(p >= 0.0 && p <= 1.0)) throw DataFrameError(DataFrameError::ComputeError, "percentile: p must lie in [0, 1]");
            calls.push_back(rdf_percentile_call{RDF_PCT_CONT, 0, p});
        }
        std::vector<std::optional<double>> out(ps.size());
        if (c.num_rows() == 0 || ps.empty()) return out;
        const DataFrame::PercentileGroups g = DataFrame::from_columns({c}).percentile_groups({}, c.name(), calls);
        for (size_t i = 0; i < ps.size() && g.groups; ++i)
            if (g.outs[i]->null_count == 0) out[i] = g.outs[i]->values_to_host<double>()[0];
        return out;
    }
    static std::optional<double> percentile(const Column& c, double p) { return percentiles(c, {p})[0]; }
    static std::optional<double> median(const Column& c) { return percentile(c, 0.5); }
    static std::optional<Column> percentile_disc(const Column& c, double p) {
        if (!(p >= 0.0 && p <= 1.0)) throw DataFrameError(DataFrameError::ComputeError, "percentile_disc: p must lie in [0, 1]");
        if (c.num_rows() == 0) return std::nullopt;
        const DataFrame::PercentileGroups g = DataFrame::from_columns({c}).percentile_groups({}, c.name(), {rdf_percentile_call{RDF_PCT_DISC, 0, p}});
        if (!g.groups || g.outs[0]->null_count > 0) return std::nullopt;
        return c.take(g.outs[0], 4096);
    }

  private:
    static std::optional<Column> first_or_last(const Column& c, int32_t fn, bool ignore_nulls) {
        if (c.num_rows() == 0) return std::nullopt;
        const std::string name = c.name();
        const DataFrame::SortedGroups g = DataFrame::from_columns({c}).sorted_groups({}, &name, {rdf_group_call{fn, ignore_nulls ? 1 : 0}});
        if (!g.groups || g.outs[0]->null_count > 0) return std::nullopt;
        return c.take(g.outs[0], 4096);
    }
    static std::vector<rdf_array> mask_views(const ChunkedArray* mask, size_t nchunks) {
        if (!mask) return {};
        if (mask->num_chunks() != nchunks) throw DataFrameError(DataFrameError::ComputeError, "moments: the mask's chunk count differs");
        return mask->views();
    }
};

inline std::optional<double> Column::median() const { return AggregateFunctions::median(*this); }
inline std::optional<double> Column::quantile(double p) const { return AggregateFunctions::percentile(*this, p); }

// ------------------------------------------------------------------------------------------------
// ListArray over a primitive child + ArrayFunctions (src/functions/array.rs:15-399)

struct ListArray {
    ArrayRef offsets;  // Int32 value_offsets, len() + 1 entries; its validity buffer is the LIST validity (len() bits)
    ArrayRef child;

    int64_t len() const { return offsets->length - 1; }
    ArrayRef values() const { return child; }
    DataType value_type() const { return child->dtype; }
    rdf_list_array view() const {
        rdf_list_array l;
        l.offsets = offsets->view();
        if (child->dtype == DataType::Utf8) {   // text stays on the host in this mirror: rdf_list_explode, which reads the offsets only, is the one call such a list goes to
            std::memset(&l.values, 0, sizeof l.values);
            l.values.dtype = RDF_U8;
            l.values.mem = l.offsets.mem;
        } else l.values = child->view();
        return l;
    }
    std::vector<int32_t> value_offsets() const { return offsets->values_to_host<int32_t>(); }
    int32_t value_offset(int64_t i) const { return offsets->value<int32_t>(i); }
    int32_t value_length(int64_t i) const { return offsets->value<int32_t>(i + 1) - offsets->value<int32_t>(i); }
    bool is_null(int64_t i) const { return offsets->validity && !offsets->bits_to_host(offsets->validity)[(size_t)i]; }

    // ArrayData::builder(List(..)).add_buffer(value_offsets).add_child_data(values) of the reference's tests (array.rs:433-440)
    static ListArray from_parts(const std::vector<int32_t>& value_offsets, ArrayRef values, const std::vector<bool>* valid = nullptr) {
        return ListArray{Array::from_vec<int32_t>(value_offsets, valid), std::move(values)};
    }
    template <class T>
    static ListArray from_rows(const std::vector<std::optional<std::vector<T>>>& rows) {
        std::vector<int32_t> off{0};
        std::vector<T> vals;
        std::vector<bool> valid;
        bool any_null = false;
        for (auto& r : rows) {
            valid.push_back(r.has_value());
            any_null |= !r.has_value();
            if (r) vals.insert(vals.end(), r->begin(), r->end());
            off.push_back((int32_t)vals.size());
        }
        return from_parts(off, Array::from_vec<T>(vals), any_null ? &valid : nullptr);
    }
    template <class T>
    std::vector<std::vector<T>> rows_to_host() const {
        const auto off = value_offsets();
        const auto vals = child->values_to_host<T>();
        std::vector<std::vector<T>> out;
        for (size_t i = 0; i + 1 < off.size(); ++i) out.emplace_back(vals.begin() + off[i], vals.begin() + off[i + 1]);
        return out;
    }
};

// Column::split / split_regexp and their ScalarFunctions (rdf_utf8_split / rdf_utf8_regexp_split): the sizing call, then the call
// into exactly sized host buffers; the chunks' lists are joined into one ListArray whose child is one Utf8 array.
template <class Call> inline ListArray Column::split_lists(const char* what, Call split_call) const {
    need_text(what);
    const TextChunks tc = text_chunks(what);
    const size_t n = tc.txt.size();
    std::vector<std::vector<int32_t>> lo(n), eo(n);
    std::vector<std::vector<uint8_t>> valid(n), data(n);
    std::vector<rdf_out> ol(n), oe(n), od(n);
    const std::vector<bool> nullable = chunk_nullable();
    for (size_t i = 0; i < n; ++i) {
        const int64_t rows = tc.txt[i].offsets.length - 1;
        lo[i].assign((size_t)rows + 1, 0);
        if (nullable[i]) valid[i].assign((size_t)((rows + 63) / 64 * 8 + 8), 0);
        ol[i] = rdf_out{lo[i].data(), nullable[i] ? valid[i].data() : nullptr, rows + 1, 0, 0, RDF_I32, RDF_MEM_HOST};
        oe[i] = rdf_out{nullptr, nullptr, 0, 0, 0, RDF_I32, RDF_MEM_HOST};
        od[i] = rdf_out{nullptr, nullptr, 0, 0, 0, RDF_U8, RDF_MEM_HOST};
    }
    auto call = [&] { return split_call(tc.txt.data(), (int64_t)n, ol.data(), oe.data(), od.data()); };
    rdf_status st = call();
    if (st == RDF_MEMORY_ERROR && n > 0 && oe[0].length > 0) {
        for (size_t i = 0; i < n; ++i) {
            eo[i].assign((size_t)oe[i].length, 0);
            oe[i].values = eo[i].data();
            oe[i].capacity = oe[i].length;
            data[i].assign((size_t)od[i].length + 8, 0);
            od[i].values = data[i].data();
            od[i].capacity = od[i].length;
        }
        st = call();
    }
    check(st);
    std::vector<int32_t> offsets{0};
    std::vector<std::string> strs;
    std::vector<bool> ok;
    bool any_null = false;
    for (size_t i = 0; i < n; ++i) {
        const int64_t rows = ol[i].length - 1;
        for (int64_t r = 0; r < rows; ++r) {
            const bool bit = !nullable[i] || ((valid[i][(size_t)(r >> 3)] >> (r & 7)) & 1);
            ok.push_back(bit);
            any_null |= !bit;
            for (int32_t e = lo[i][(size_t)r]; e < lo[i][(size_t)r + 1]; ++e)
                strs.emplace_back((const char*)data[i].data() + eo[i][(size_t)e], (size_t)(eo[i][(size_t)e + 1] - eo[i][(size_t)e]));
            offsets.push_back((int32_t)strs.size());
        }
    }
    return ListArray::from_parts(offsets, Array::from_strings(std::move(strs)), any_null ? &ok : nullptr);
}
inline ListArray Column::split(const std::string& delim, int64_t limit) const {
    return split_lists("split", [&](const rdf_utf8_array* c, int64_t n, rdf_out* ol, rdf_out* oe, rdf_out* od) {
        return rdf_utf8_split(c, n, (const uint8_t*)delim.data(), (int64_t)delim.size(), limit, ol, oe, od);
    });
}
inline ListArray Column::split_regexp(const std::string& pattern, int64_t limit) const {
    return split_lists("split_regexp", [&](const rdf_utf8_array* c, int64_t n, rdf_out* ol, rdf_out* oe, rdf_out* od) {
        return rdf_utf8_regexp_split(c, n, (const uint8_t*)pattern.data(), (int64_t)pattern.size(), limit, ol, oe, od);
    });
}
inline ListArray ScalarFunctions::split(const std::vector<ArrayRef>& arr, const std::string& delim, int64_t limit) { return text_column(arr, "split").split(delim, limit); }
inline ListArray ScalarFunctions::split_regexp(const std::vector<ArrayRef>& arr, const std::string& pattern, int64_t limit) {
    return text_column(arr, "split_regexp").split_regexp(pattern, limit);
}

struct ArrayFunctions {
    // array.rs:15-37: NULL list -> NULL, else whether the row's slice holds `val`
    template <class T> static ArrayRef array_contains(const ListArray& array, T val) {
        expect_child<T>(array, "array_contains");
        auto out = Array::make_out(DataType::Boolean, array.len(), true);
        return one(array, out, [&](const rdf_list_array* l, rdf_out* o) { return rdf_list_contains(l, &val, o); });
    }
    // array.rs:233-260: 1-based position of the first match, 0 when absent or the list is NULL
    template <class T> static ArrayRef array_position(const ListArray& array, T val) {
        expect_child<T>(array, "array_position");
        auto out = Array::make_out(DataType::Int32, array.len(), false);
        return one(array, out, [&](const rdf_list_array* l, rdf_out* o) { return rdf_list_position(l, &val, o); });
    }
    // array.rs:182-231
    template <class T> static ArrayRef array_max(const ListArray& array) {
        expect_child<T>(array, "array_max");
        auto out = Array::make_out(array.value_type(), array.len(), true);
        return one(array, out, [&](const rdf_list_array* l, rdf_out* o) { return rdf_list_max(l, o); });
    }
    template <class T> static ArrayRef array_min(const ListArray& array) {
        expect_child<T>(array, "array_min");
        auto out = Array::make_out(array.value_type(), array.len(), true);
        return one(array, out, [&](const rdf_list_array* l, rdf_out* o) { return rdf_list_min(l, o); });
    }
    // array.rs:262-292
    template <class T> static ListArray array_remove(const ListArray& array, T val) {
        expect_child<T>(array, "array_remove");
        return rebuild(array, array.child->length, [&](const rdf_list_array* l, rdf_out* oo, rdf_out* ov) { return rdf_list_remove(l, &val, oo, ov); });
    }
    // array.rs:39-65
    template <class T> static ListArray array_distinct(const ListArray& array) {
        expect_child<T>(array, "array_distinct");
        return rebuild(array, array.child->length, [&](const rdf_list_array* l, rdf_out* oo, rdf_out* ov) { return rdf_list_distinct(l, oo, ov); });
    }
    // array.rs:66-153,356-399
    template <class T> static ListArray array_except(const ListArray& a, const ListArray& b) {
        expect_child<T>(a, "array_except");
        const rdf_list_array lb = b.view();
        return rebuild(a, a.child->length, [&](const rdf_list_array* l, rdf_out* oo, rdf_out* ov) { return rdf_list_except(l, &lb, oo, ov); });
    }
    template <class T> static ListArray array_intersect(const ListArray& a, const ListArray& b) {
        expect_child<T>(a, "array_intersect");
        const rdf_list_array lb = b.view();
        return rebuild(a, a.child->length, [&](const rdf_list_array* l, rdf_out* oo, rdf_out* ov) { return rdf_list_intersect(l, &lb, oo, ov); });
    }
    template <class T> static ListArray array_union(const ListArray& a, const ListArray& b) {
        expect_child<T>(a, "array_union");
        const rdf_list_array lb = b.view();
        return rebuild(a, a.child->length + b.child->length, [&](const rdf_list_array* l, rdf_out* oo, rdf_out* ov) { return rdf_list_union(l, &lb, oo, ov); });
    }
    // array.rs:294-326
    template <class T> static ListArray array_repeat(const ListArray& array, int32_t count) {
        expect_child<T>(array, "array_repeat");
        return rebuild(array, array.child->length * (int64_t)(count > 0 ? count : 0), [&](const rdf_list_array* l, rdf_out* oo, rdf_out* ov) { return rdf_list_repeat(l, count, oo, ov); });
    }
    // array.rs:328-354: the value_offsets stay, every slice ascending
    template <class T> static ListArray array_sort(const ListArray& array) {
        expect_child<T>(array, "array_sort");
        auto off = array.value_offsets();
        const int64_t total = off.empty() ? 0 : (int64_t)off.back() - off.front();
        auto vals = Array::make_out(array.value_type(), total, false);
        const rdf_list_array l = array.view();
        rdf_out ov = vals->out_view(total);
        check(rdf_list_sort(&l, &ov));
        vals->length = ov.length;
        const int32_t first = off.empty() ? 0 : off.front();
        for (auto& o : off) o -= first;   // the sorted values start at the first row's slice
        std::vector<bool> valid;
        if (array.offsets->validity) valid = array.offsets->bits_to_host(array.offsets->validity), valid.resize((size_t)array.len());
        return ListArray::from_parts(off, vals, array.offsets->validity ? &valid : nullptr);
    }

    // collect_list() / collect_set() (array.rs:404-405, declared with empty bodies: Spark's semantics, written down at
    // rdf_groupby_collect) of a whole numeric column, no grouping: a ONE-row ListArray of the non-NULL values in row order
    // (list), or of the distinct non-NULL values ascending, floats canonical (set).  An empty or all-NULL column gives one
    // empty list.  Per group: Evaluate::group_collect.
    static ListArray collect_list(const Column& c) { return collect(c, RDF_COLLECT_LIST); }
    static ListArray collect_set(const Column& c) { return collect(c, RDF_COLLECT_SET); }

  private:
    static ListArray collect(const Column& c, int32_t kind) {
        if (c.data_type() == DataType::Utf8 || c.data_type() == DataType::Boolean)
            throw DataFrameError(DataFrameError::ComputeError, "collect: a ListArray holds a numeric child (Utf8: Evaluate::group_collect)");
        const DataFrame::CollectedGroups g = DataFrame::from_columns({c}).collected_groups({}, c.name(), kind);
        return ListArray::from_parts({0, (int32_t)g.elements}, g.values);
    }
    template <class T> static void expect_child(const ListArray& a, const char* fn) {
        if (a.value_type() != TypeOf<T>::value) throw DataFrameError(DataFrameError::ComputeError, std::string(fn) + ": the list's value type is not the requested one");
    }
    template <class F> static ArrayRef one(const ListArray& array, std::shared_ptr<Array> out, F call) {
        const rdf_list_array l = array.view();
        rdf_out o = out->out_view(array.len());
        check(call(&l, &o));
        out->length = o.length;
        out->null_count = o.null_count;
        return out;
    }
    template <class F> static ListArray rebuild(const ListArray& array, int64_t capacity, F call) {
        auto off = Array::make_out(DataType::Int32, array.len() + 1, false);
        auto vals = Array::make_out(array.value_type(), capacity, false);
        const rdf_list_array l = array.view();
        rdf_out oo = off->out_view(array.len() + 1), ov = vals->out_view(capacity);
        check(call(&l, &oo, &ov));
        off->length = oo.length;
        vals->length = ov.length;
        return ListArray{off, vals};
    }
};

inline DataFrame ScalarFunctions::explode_rows(const DataFrame& frame, const ListArray& list, const std::string* pos_name, const std::string& name, bool outer) {
    if (frame.num_columns() > 0 && (int64_t)frame.num_rows() != list.len())
        throw DataFrameError(DataFrameError::ComputeError, "explode: the list column and the frame differ in length");
    const bool host = list.offsets->host;
    const rdf_list_array l = list.view();
    int64_t rows = 0;
    check(rdf_list_explode(&l, outer ? 1 : 0, nullptr, nullptr, nullptr, &rows));          // the count-only call sizes the outputs
    auto parent = Array::make_out(DataType::UInt32, rows, false, host), child = Array::make_out(DataType::UInt32, rows, outer, host);
    auto pos = pos_name ? Array::make_out(DataType::Int32, rows, outer, host) : nullptr;
    rdf_out op = parent->out_view(rows), oc = child->out_view(rows), opos{};
    if (pos) opos = pos->out_view(rows);
    check(rdf_list_explode(&l, outer ? 1 : 0, &op, &oc, pos ? &opos : nullptr, &rows));
    parent->length = op.length;
    child->length = oc.length; child->null_count = oc.null_count;
    if (oc.null_count == 0) child->validity = nullptr;
    if (pos) { pos->length = opos.length; pos->null_count = opos.null_count; if (opos.null_count == 0) pos->validity = nullptr; }
    DataFrame out = frame.take(parent);
    if (pos) out = out.with_column(*pos_name, Column::from_arrays({pos}, Field{*pos_name, DataType::Int32, true}));
    const Column elements = Column::from_arrays({list.child}, Field{name, list.value_type(), true});
    return out.with_column(name, elements.take(child, 4096));
}
inline DataFrame ScalarFunctions::explode(const DataFrame& frame, const ListArray& list, const std::string& name, bool outer) { return explode_rows(frame, list, nullptr, name, outer); }
inline DataFrame ScalarFunctions::explode_outer(const DataFrame& frame, const ListArray& list, const std::string& name) { return explode_rows(frame, list, nullptr, name, true); }
inline DataFrame ScalarFunctions::posexplode(const DataFrame& frame, const ListArray& list, const std::string& pos_name, const std::string& name, bool outer) {
    return explode_rows(frame, list, &pos_name, name, outer);
}

// What Evaluate::group_collect returns: one List row per group, for a numeric and for a Utf8 value column alike.
//   keys     the grouping columns gathered by every group's first row: ascending, the NULL group last (no columns when the
//            call had no grouping columns: one group)
//   offsets  Int32, groups + 1 entries starting at 0; every list is valid, a group without a non-NULL value has an empty one
//   child    the elements, ONE chunk named and typed like the value column: numeric (collect_set: floats canonical) or Utf8
//            (the mirror keeps text on the host and gathers it there by the element rows the call returns)
// lists(): the (offsets, child) pair as a ListArray, for a numeric child.
struct GroupedLists {
    DataFrame keys;
    ArrayRef offsets;
    Column child;
    int64_t groups() const { return offsets->length - 1; }
    ListArray lists() const {
        if (child.data_type() == DataType::Utf8) throw DataFrameError(DataFrameError::ComputeError, "a ListArray holds a numeric child");
        return ListArray{offsets, child.data().chunks().at(0)};
    }
};

// ------------------------------------------------------------------------------------------------
// Evaluate (src/evaluation.rs:54-323), fusing

inline int32_t scalar_function_op(plan::ScalarFunction f) {
    using SF = plan::ScalarFunction;
    switch (f) {
        case SF::Add: return RDF_OP_ADD; case SF::Subtract: return RDF_OP_SUB; case SF::Multiply: return RDF_OP_MUL;
        case SF::Divide: return RDF_OP_DIV; case SF::Abs: return RDF_OP_ABS; case SF::Sine: return RDF_OP_SIN;
        case SF::Cosine: return RDF_OP_COS; case SF::Tangent: return RDF_OP_TAN;
        case SF::Cotangent: return RDF_OP_COT; case SF::Secant: return RDF_OP_SEC; case SF::Cosecant: return RDF_OP_CSC;
        default: throw DataFrameError(DataFrameError::ComputeError, std::string("Scalar Function ") + plan::scalar_function_name(f) + " not supported");
    }
}

class Evaluate {
  public:
    // Evaluate::calculate, eager: ONE Calculation materialised as a new column (drop-in for :97-323)
    static DataFrame calculate(const DataFrame& frame, const plan::Calculation& calc) {
        Evaluate ev(frame);
        ev.step_calculate(calc);
        return ev.flush();
    }
    // collect_list / collect_set per group (ArrayFunction::CollectList / CollectSet, src/expression.rs:691-692): one
    // rdf_groupby_collect over 0..4 grouping columns, numeric or Utf8, and ONE value column, numeric or Utf8.  The groups come
    // in the order group_aggregate puts its rows into, so the two line up row for row.  The plan's GroupAggregate keeps its
    // set of aggregations: the reference files these two under ArrayFunction, not AggregateFunction.
    static GroupedLists group_collect(const DataFrame& frame, const std::vector<std::string>& groups, const std::string& column, int32_t kind) {
        const DataFrame::CollectedGroups g = frame.collected_groups(groups, column, kind);
        const Column& vc = frame.column_by_name(column);
        std::vector<Column> keys;
        for (auto& n : groups) {
            const Column& kc = frame.column_by_name(n);
            keys.push_back(Column::from_arrays(kc.take(g.group_rows, 4096).data().chunks(), Field{n, kc.data_type(), true}));
        }
        Column child = g.values ? Column::from_arrays({g.values}, Field{column, vc.data_type(), true})
                                : Column::from_arrays(vc.take(g.child_rows, 4096).data().chunks(), Field{column, vc.data_type(), true});
        return GroupedLists{DataFrame::from_columns(std::move(keys)), g.offsets, std::move(child)};
    }
    // Percentiles per group, eager (the planner's AggregateFunction enum has no percentile): the grouping columns — 0 .. 4 of
    // them, integer, float or Utf8, gathered through the groups' first rows — then one column per call.  A continuous call
    // {RDF_PCT_CONT, 0, p} gives the Float64 column "percentile(x, p)" ("median(x)" for p = 0.5), a discrete one
    // {RDF_PCT_DISC, 0, p} the column "percentile_disc(x, p)" typed like x (numeric or Utf8), taken by the row indices the call
    // returns.  Rows ordered by the grouping columns, the NULL group last; a group without a non-NULL x has NULL in every column.
    static DataFrame group_percentile(const DataFrame& frame, const std::vector<std::string>& groups, const std::string& value,
                                      const std::vector<rdf_percentile_call>& calls) {
        if (groups.size() > RDF_MAX_GROUP_KEYS) throw DataFrameError(DataFrameError::ComputeError, "group_percentile: at most " + std::to_string(RDF_MAX_GROUP_KEYS) + " grouping columns");
        if (calls.empty() || calls.size() > RDF_PERCENTILE_MAX_CALLS) throw DataFrameError(DataFrameError::ComputeError, "group_percentile: 1.." + std::to_string(RDF_PERCENTILE_MAX_CALLS) + " calls");
        const Column& vc = frame.column_by_name(value);
        const DataFrame::PercentileGroups g = frame.percentile_groups(groups, value, calls);
        std::vector<Column> out_cols;
        for (auto& n : groups) {
            const Column& kc = frame.column_by_name(n);
            out_cols.push_back(Column::from_arrays(kc.take(g.group_rows, 4096).data().chunks(), Field{n, kc.data_type(), true}));
        }
        auto p_text = [](double p) { std::ostringstream o; o << p; return o.str(); };
        for (size_t c = 0; c < calls.size(); ++c) {
            if (calls[c].kind == RDF_PCT_CONT) {
                const std::string name = calls[c].p == 0.5 ? "median(" + value + ")" : "percentile(" + value + ", " + p_text(calls[c].p) + ")";
                out_cols.push_back(Column::from_arrays({g.outs[c]}, Field{name, DataType::Float64, true}));
                continue;
            }
            // the value column taken by the calls' row indices; where the call is NULL the index is 0, and the row is masked
            Column taken = vc.take(g.outs[c], 4096);
            out_cols.push_back(Column::from_arrays(taken.data().chunks(), Field{"percentile_disc(" + value + ", " + p_text(calls[c].p) + ")", vc.data_type(), true}));
        }
        return DataFrame::from_columns(std::move(out_cols));
    }
    // Variance, stddev, skewness, kurtosis (and the mean) per group, eager: the grouping columns — 0 .. 4 of them, integer,
    // float or Utf8, gathered through the groups' first rows — then one nullable Float64 column per statistic (rdf_stat), named
    // mean(x), var_pop(x), var_samp(x), stddev_pop(x), stddev_samp(x), skewness(x), kurtosis(x).  ONE rdf_groupby_moments call,
    // whose sort is over the grouping columns alone.  Rows ordered by the grouping columns, the NULL group last; a statistic
    // that is absent (no non-NULL x, a sample form of one row, skewness / kurtosis of a constant group) is NULL.
    static DataFrame group_moments(const DataFrame& frame, const std::vector<std::string>& groups, const std::string& value, const std::vector<int32_t>& stats) {
        static const char* names[] = {"mean", "var_pop", "var_samp", "stddev_pop", "stddev_samp", "skewness", "kurtosis"};
        std::vector<std::string> cols;
        for (int32_t st : stats) {
            if (st < RDF_STAT_MEAN || st > RDF_STAT_KURTOSIS) throw DataFrameError(DataFrameError::ComputeError, "group_moments: unknown statistic " + std::to_string(st));
            cols.push_back(std::string(names[st]) + "(" + value + ")");
        }
        return group_moments_frame(frame, groups, value, nullptr, stats, cols, "group_moments");
    }
    // covar_pop / covar_samp / corr of (x, y) per group (rdf_costat): as group_moments; a row counts when both values are not
    // NULL.  The columns are covar_pop(x, y), covar_samp(x, y), corr(x, y).
    static DataFrame group_comoments(const DataFrame& frame, const std::vector<std::string>& groups, const std::string& x, const std::string& y,
                                     const std::vector<int32_t>& costats) {
        static const char* names[] = {"covar_pop", "covar_samp", "corr"};
        std::vector<std::string> cols;
        for (int32_t st : costats) {
            if (st < RDF_COSTAT_COVAR_POP || st > RDF_COSTAT_CORR) throw DataFrameError(DataFrameError::ComputeError, "group_comoments: unknown statistic " + std::to_string(st));
            cols.push_back(std::string(names[st]) + "(" + x + ", " + y + ")");
        }
        return group_moments_frame(frame, groups, x, &y, costats, cols, "group_comoments");
    }
    static DataFrame group_moments_frame(const DataFrame& frame, const std::vector<std::string>& groups, const std::string& x, const std::string* y,
                                         const std::vector<int32_t>& stats, const std::vector<std::string>& cols, const char* what) {
        if (groups.size() > RDF_MAX_GROUP_KEYS) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": at most " + std::to_string(RDF_MAX_GROUP_KEYS) + " grouping columns");
        if (stats.empty() || stats.size() > RDF_GROUP_MOMENTS_MAX_CALLS) throw DataFrameError(DataFrameError::ComputeError, std::string(what) + ": 1.." + std::to_string(RDF_GROUP_MOMENTS_MAX_CALLS) + " statistics");
        std::vector<rdf_group_stat_call> calls;
        for (int32_t st : stats) calls.push_back(rdf_group_stat_call{st, 0});
        const DataFrame::MomentGroups g = frame.moment_groups(groups, x, y, calls);
        std::vector<Column> out_cols;
        for (auto& n : groups) {
            const Column& kc = frame.column_by_name(n);
            out_cols.push_back(Column::from_arrays(kc.take(g.group_rows, 4096).data().chunks(), Field{n, kc.data_type(), true}));
        }
        for (size_t c = 0; c < calls.size(); ++c) out_cols.push_back(Column::from_arrays({g.outs[c]}, Field{cols[c], DataType::Float64, true}));
        return DataFrame::from_columns(std::move(out_cols));
    }
    // GROUP BY, eager, over 1..4 grouping columns of which each is an integer or a Utf8 column: the grouping columns, then one
    // column per (aggregation, input column), named and typed as Dataset::try_aggregate plans them; rows ordered by the
    // grouping columns, text in byte order, the NULL group last.  Integer columns only: the GroupAggregate step of a plan,
    // unchanged.  With a text column the keys are dictionary-encoded on the device (rdf_groupby_agg_keys).  The lazy plan's
    // GroupAggregate step itself keeps refusing text columns, as the reference's evaluation does.
    static DataFrame group_aggregate(const DataFrame& frame, const std::vector<std::string>& groups, const std::vector<plan::Aggregation>& aggregations) {
        plan::Transformation t;
        t.kind = plan::Transformation::GroupAggregate;
        t.names = groups;
        t.aggregations = aggregations;
        if (groups.empty() || groups.size() > RDF_MAX_GROUP_KEYS)
            throw DataFrameError(DataFrameError::ComputeError, "GroupAggregate: 1.." + std::to_string(RDF_MAX_GROUP_KEYS) + " grouping columns");
        bool any_text = false;
        for (auto& n : groups) any_text |= frame.column_by_name(n).data_type() == DataType::Utf8;
        if (any_text) return group_aggregate_text(frame, t);
        Evaluate ev(frame);
        ev.step_group_aggregate(t);
        return ev.flush();
    }
    // Evaluate::evaluate (:66-96): computations newest-first (Expression::unroll order), each applied to
    // the running frame.  Calculate / Filter / Select / Drop / Rename stay lazy and are flushed as fused
    // passes; Limit and the end of the plan materialise; GroupAggregate with no groups is the fused
    // filter -> aggregate pass.
    static DataFrame evaluate(const DataFrame& frame, const std::vector<plan::Computation>& comps) {
        Evaluate ev(frame);
        for (auto c = comps.rbegin(); c != comps.rend(); ++c)
            for (auto& t : c->transformations) ev.step(t);
        return ev.flush();
    }

  private:
    struct Lazy { std::string name; DataType dtype; ExprRef def; };  // def == nullptr: column `source` of base_
    struct Entry { std::string name; DataType dtype; ExprRef def; std::string source; };

    explicit Evaluate(const DataFrame& f) : base_(f) {
        for (auto& fld : f.schema().fields) cols_.push_back(Entry{fld.name, fld.data_type, nullptr, fld.name});
    }
    Entry* find(const std::string& n) { for (auto& e : cols_) if (e.name == n) return &e; return nullptr; }
    ExprRef ref(const std::string& n) {
        Entry* e = find(n);
        if (!e) throw DataFrameError(DataFrameError::ComputeError, "Column not found by name: " + n);
        return e->def ? e->def : Expr::col(e->source);
    }
    void put(const std::string& name, DataType dt, ExprRef def) {  // with_column: replace-at-end semantics
        for (size_t i = 0; i < cols_.size(); ++i) if (cols_[i].name == name) { cols_.erase(cols_.begin() + i); break; }
        cols_.push_back(Entry{name, dt, std::move(def), ""});
    }

    void step(const plan::Transformation& t) {
        using T = plan::Transformation;
        switch (t.kind) {
            case T::Calculate: step_calculate(t.calc); break;
            case T::Filter: step_filter(t.filter); break;
            case T::Limit:
                // the optimiser's limit push-down (src/optimiser.rs:56-75): pending Calculate steps are row-wise, so the limit
                // is taken on the source columns (zero-copy slices) and the lazy columns are then computed for those rows only;
                // a pending filter changes which rows come first, so it is applied before the limit
                if (!pending_) base_ = base_.limit(t.limit);
                else { DataFrame f = flush(); reset(f.limit(t.limit)); }
                break;
            case T::Select: {
                std::vector<Entry> keep;
                for (auto& e : cols_) for (auto& n : t.names) if (e.name == n) { keep.push_back(e); break; }
                cols_ = keep;
            } break;
            case T::Drop: {
                std::vector<Entry> keep;
                for (auto& e : cols_) { bool d = false; for (auto& n : t.names) d |= e.name == n; if (!d) keep.push_back(e); }
                cols_ = keep;
            } break;
            case T::GroupAggregate: step_aggregate(t); break;
            case T::Sort: {
                DataFrame f = flush();
                std::vector<DataFrame::SortCriteria> cr;
                for (auto& n : t.names) cr.push_back(DataFrame::SortCriteria{n, false, false});
                for (size_t i = 0; i < t.sort_descending.size() && i < cr.size(); ++i) cr[i].descending = t.sort_descending[i];
                reset(f.sort(cr));
            } break;
            case T::Join: throw DataFrameError(DataFrameError::ComputeError, "Join inside a computation list: LazyFrame::join evaluates both sides and joins the frames");
            default: throw DataFrameError(DataFrameError::ComputeError, "Read inside evaluate: pass the frame in");
        }
    }

    void step_calculate(const plan::Calculation& calc) {
        using F = plan::Function;
        std::vector<ExprRef> in;
        for (auto& c : calc.inputs) in.push_back(ref(c.name));
        switch (calc.function.kind) {
            case F::Scalar: {
                const DataType dt = calc.output.data_type;
                const auto sf = calc.function.scalar;
                const bool binary = sf == plan::ScalarFunction::Add || sf == plan::ScalarFunction::Subtract || sf == plan::ScalarFunction::Multiply || sf == plan::ScalarFunction::Divide;
                if (binary) {
                    if (dt == DataType::Int8 || dt == DataType::UInt8 || dt == DataType::Boolean || dt == DataType::Utf8)
                        throw DataFrameError(DataFrameError::ComputeError, "Unsupported operation");  // evaluation.rs:239
                    if (in.size() != 2) throw DataFrameError(DataFrameError::ComputeError, "binary scalar function expects 2 inputs");
                    if (sf == plan::ScalarFunction::Divide && pending_) { DataFrame f = flush(); reset(f); in = {ref(calc.inputs[0].name), ref(calc.inputs[1].name)}; }
                    put(calc.output.name, dt, Expr::make(scalar_function_op(sf), in[0], in[1]));
                } else {
                    if (!is_float(dt)) throw DataFrameError(DataFrameError::ComputeError, std::string("Expecting float datatype for operation, found ") + type_name(dt));  // :282-284
                    put(calc.output.name, dt, Expr::make(scalar_function_op(sf), in[0]));
                }
            } break;
            case F::Cast: put(calc.output.name, calc.output.data_type, Expr::make(RDF_OP_CAST, in[0], nullptr, (int32_t)calc.output.data_type)); break;
            case F::Rename: {
                Entry* e = find(calc.inputs[0].name);
                if (!e) throw DataFrameError(DataFrameError::NoneError, "column " + calc.inputs[0].name + " not found");
                e->name = calc.output.name;
            } break;
            case F::Filter: step_filter(calc.function.filter); break;
        }
    }
    void step_filter(const FilterRef& f) {
        ExprRef p = filter_to_expr(f, [this](const std::string& n) { return ref(n); });
        pending_ = pending_ ? Expr::make(RDF_OP_AND, pending_, p) : p;
    }

    // fused filter -> aggregates (GroupAggregate with no grouping columns)
    // GroupAggregate WITH grouping columns: the reference plans it (Dataset::try_aggregate, src/expression.rs:114-221)
    // and panics on execution (src/evaluation.rs:73).  Here: one integer grouping column, Sum / Count / Avg per group
    // through rdf_groupby_sum; rows of the result are ordered by key (NULL group last) so every aggregate column lines up.
    // Utf8 grouping columns, alone or next to integer ones, go through Evaluate::group_aggregate (rdf_groupby_agg_keys).

    // One aggregate column of a GROUP BY result from the per-group sums (or extrema) and counts, already in result order.
    static void append_aggregate_column(plan::AggregateFunction fn, const std::string& col, DataType vdt, DataType sdt, const std::vector<ArrayRef>& sums,
                                        const std::vector<ArrayRef>& counts, std::vector<Column>& out_cols) {
        using AF = plan::AggregateFunction;
        if (fn == AF::Sum) {
            out_cols.push_back(Column::from_arrays(sdt == vdt ? sums : ScalarFunctions::cast(sums, vdt), Field{"sum(" + col + ")", vdt, true}));
        } else if (fn == AF::Min || fn == AF::Max) {   // typed like the input (try_aggregate): the extremum of a group always fits
            out_cols.push_back(Column::from_arrays(sdt == vdt ? sums : ScalarFunctions::cast(sums, vdt), Field{std::string(fn == AF::Min ? "min(" : "max(") + col + ")", vdt, true}));
        } else if (fn == AF::Count) {
            out_cols.push_back(Column::from_arrays(ScalarFunctions::cast(counts, DataType::UInt32), Field{"count(" + col + ")", DataType::UInt32, true}));
        } else {   // avg = sum / count, NULL for a group without a non-null value (AggregateFunctions::avg, src/functions/aggregate.rs:32-65)
            std::vector<ArrayRef> out;
            const std::vector<ArrayRef> fs = sdt == DataType::Float64 ? sums : ScalarFunctions::cast(sums, DataType::Float64);
            for (size_t i = 0; i < fs.size(); ++i) {
                const std::vector<double> sv = fs[i]->values_to_host<double>();
                const std::vector<int64_t> cv = counts[i]->values_to_host<int64_t>();
                std::vector<double> m(sv.size());
                std::vector<bool> valid(sv.size());
                for (size_t r = 0; r < sv.size(); ++r) { valid[r] = cv[r] > 0; m[r] = cv[r] > 0 ? sv[r] / (double)cv[r] : 0.0; }
                out.push_back(Array::from_vec(m, &valid));
            }
            out_cols.push_back(Column::from_arrays(out, Field{"avg(" + col + ")", DataType::Float64, true}));
        }
    }

    // CountDistinct / First / Last of one column per group: one rdf_groupby_sorted (one sort over the grouping columns and the
    // column), whose groups come in ascending key order with the NULL group last — the order every other aggregate column of
    // the step is put into, so the rows line up.  count_distinct(x) is UInt32 like count(x); first(x) / last(x) are typed like
    // x (numeric or Utf8) and gathered by the row indices the call returns: the first / last row of the group, NULL if x is.
    static void append_sorted_aggregate(const DataFrame& f, const std::vector<std::string>& names, plan::AggregateFunction fn, const std::string& col,
                                        std::vector<Column>& out_cols) {
        using AF = plan::AggregateFunction;
        const Column& vc = f.column_by_name(col);
        const int32_t gfn = fn == AF::CountDistinct ? RDF_GRP_COUNT_DISTINCT : fn == AF::First ? RDF_GRP_FIRST : RDF_GRP_LAST;
        const DataFrame::SortedGroups g = f.sorted_groups(names, &col, {rdf_group_call{gfn, 0}});
        if (out_cols.empty())
            for (auto& n : names) {
                const Column& kc = f.column_by_name(n);
                out_cols.push_back(Column::from_arrays(kc.take(g.group_rows, 4096).data().chunks(), Field{n, kc.data_type(), true}));
            }
        if (fn == AF::CountDistinct) {
            out_cols.push_back(Column::from_arrays(ScalarFunctions::cast({g.outs[0]}, DataType::UInt32), Field{"count_distinct(" + col + ")", DataType::UInt32, true}));
            return;
        }
        out_cols.push_back(Column::from_arrays(vc.take(g.outs[0], 4096).data().chunks(), Field{std::string(fn == AF::First ? "first(" : "last(") + col + ")", vc.data_type(), true}));
    }

    // Variance / StdDev / Skewness / Kurtosis of one column per group: ONE rdf_groupby_moments call per value column, carrying
    // every such statistic the step asks of it (`done` keeps the calls made), whose groups come in ascending key order with
    // the NULL group last — the order every other aggregate column of the step is put into, so the rows line up.  The sample
    // forms apply, as in AggregateFunctions::variance / stddev; the columns are variance(x), stddev(x), skewness(x),
    // kurtosis(x), Float64, NULL where the statistic is absent.
    static bool moment_function(plan::AggregateFunction fn) {
        using AF = plan::AggregateFunction;
        return fn == AF::Variance || fn == AF::StdDev || fn == AF::Skewness || fn == AF::Kurtosis;
    }
    struct MomentCalls { std::string col; std::vector<plan::AggregateFunction> fns; DataFrame::MomentGroups g; };
    static void append_moment_aggregate(const DataFrame& f, const plan::Transformation& t, plan::AggregateFunction fn, const std::string& col,
                                        std::vector<MomentCalls>& done, std::vector<Column>& out_cols) {
        using AF = plan::AggregateFunction;
        auto stat_of = [](AF a) { return a == AF::Variance ? RDF_STAT_VAR_SAMP : a == AF::StdDev ? RDF_STAT_STDDEV_SAMP : a == AF::Skewness ? RDF_STAT_SKEWNESS : RDF_STAT_KURTOSIS; };
        size_t at = 0;
        while (at < done.size() && done[at].col != col) ++at;
        if (at == done.size()) {
            const DataType vdt = f.column_by_name(col).data_type();
            if (!(is_integer(vdt) || is_float(vdt))) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column must be numeric");
            MomentCalls m;
            m.col = col;
            for (auto& a : t.aggregations)
                if (moment_function(a.function) && std::find(a.columns.begin(), a.columns.end(), col) != a.columns.end() &&
                    std::find(m.fns.begin(), m.fns.end(), a.function) == m.fns.end())
                    m.fns.push_back(a.function);
            std::vector<rdf_group_stat_call> calls;
            for (AF a : m.fns) calls.push_back(rdf_group_stat_call{stat_of(a), 0});
            m.g = f.moment_groups(t.names, col, nullptr, calls);
            done.push_back(std::move(m));
        }
        const MomentCalls& m = done[at];
        if (out_cols.empty())
            for (auto& n : t.names) {
                const Column& kc = f.column_by_name(n);
                out_cols.push_back(Column::from_arrays(kc.take(m.g.group_rows, 4096).data().chunks(), Field{n, kc.data_type(), true}));
            }
        const size_t c = (size_t)(std::find(m.fns.begin(), m.fns.end(), fn) - m.fns.begin());
        const char* name = fn == AF::Variance ? "variance(" : fn == AF::StdDev ? "stddev(" : fn == AF::Skewness ? "skewness(" : "kurtosis(";
        out_cols.push_back(Column::from_arrays({m.g.outs[c]}, Field{std::string(name) + col + ")", DataType::Float64, true}));
    }

    // A step with two or more hash aggregations (Sum / Min / Max / Count / Avg) over a device-resident frame: ONE
    // rdf_groupby_multi call — the keys prepared and hashed once, every aggregate folded into one table, all outputs in one
    // group order — and ONE sort of the groups for all columns, instead of a hash GROUP BY and a sort per aggregation.  Avg
    // comes from the sum and the count of its call; Sum and Avg of one column share a call.  The promise is
    // rdf_groupby_multi_capacity(ncalls), what the one-pass route holds.  -> false, with out_cols untouched, when the step is
    // not of that shape (one hash aggregation, host-resident columns, more than 8 calls or value columns) or holds more groups
    // than the promise: the per-aggregation path then answers as before (the table route for large group counts has not been
    // measured against it).  CountDistinct / First / Last of the same step keep their sorted path; its groups come
    // in the same order.  Same column names, dtypes, order and values as the per-aggregation path.
    static bool group_aggregate_multi(const DataFrame& f, const plan::Transformation& t, const std::vector<const Column*>& kcs, bool on_host,
                                      std::vector<Column>& out_cols) {
        using AF = plan::AggregateFunction;
        auto hashed = [](AF fn) { return fn == AF::Sum || fn == AF::Min || fn == AF::Max || fn == AF::Count || fn == AF::Avg; };
        struct Entry { int32_t agg; std::string col; int value; DataType vdt, sdt; bool val_nulls; };
        std::vector<Entry> entries;
        std::vector<std::string> vcols;
        size_t nhash = 0;
        auto entry_of = [&](int32_t agg, const std::string& col) -> int {
            for (size_t i = 0; i < entries.size(); ++i) if (entries[i].agg == agg && entries[i].col == col) return (int)i;
            return -1;
        };
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) {
                if (!hashed(a.function)) {
                    if (a.function != AF::CountDistinct && a.function != AF::First && a.function != AF::Last) return false;
                    continue;
                }
                ++nhash;
                const Column& vc = f.column_by_name(c);
                const DataType vdt = vc.data_type();
                if (!(is_integer(vdt) || is_float(vdt))) return false;   // (the per-aggregation path words the refusal)
                const int32_t agg = a.function == AF::Min ? RDF_AGG_MIN : a.function == AF::Max ? RDF_AGG_MAX : a.function == AF::Count ? RDF_AGG_COUNT : RDF_AGG_SUM;
                if (entry_of(agg, c) >= 0) continue;
                size_t v = 0;
                while (v < vcols.size() && vcols[v] != c) ++v;
                if (v == vcols.size()) vcols.push_back(c);
                bool val_nulls = false;
                for (auto& ch : vc.data().chunks()) val_nulls |= ch->validity != nullptr;
                const bool extremum = agg == RDF_AGG_MIN || agg == RDF_AGG_MAX;
                const DataType sdt = agg == RDF_AGG_COUNT ? DataType::Int64 : is_float(vdt) ? DataType::Float64 : (extremum && vdt == DataType::UInt64) ? DataType::UInt64 : DataType::Int64;
                entries.push_back(Entry{agg, c, (int)v, vdt, sdt, val_nulls});
            }
        const int64_t nrows = (int64_t)f.num_rows();
        if (nhash < 2 || on_host || nrows == 0 || entries.size() > RDF_MULTI_MAX_CALLS || vcols.size() > RDF_MULTI_MAX_VALUES) return false;
        const size_t nk = kcs.size(), nch = kcs[0]->data().num_chunks(), nc = entries.size();
        std::vector<DataFrame::SortCriteria> crit;
        for (auto& n : t.names) crit.push_back(DataFrame::SortCriteria{n, false, false});
        const DataFrame::SortKeys sk = f.sort_keys(crit, false);
        std::vector<bool> key_nulls(nk, false);
        std::vector<int64_t> key_bytes(nk, 0);
        for (size_t k = 0; k < nk; ++k) {
            for (auto& a : kcs[k]->data().chunks()) if (a->validity != nullptr) key_nulls[k] = true;
            for (auto& u : sk.txt[k]) key_bytes[k] += u.data.length;
        }
        std::vector<std::vector<rdf_array>> vals(vcols.size());
        std::vector<const rdf_array*> vptr(vcols.size());
        for (size_t v = 0; v < vcols.size(); ++v) {
            for (auto& a : f.column_by_name(vcols[v]).data().chunks()) vals[v].push_back(a->view());
            vptr[v] = vals[v].data();
        }
        std::vector<rdf_multi_agg_call> calls(nc);
        for (size_t c = 0; c < nc; ++c) calls[c] = rdf_multi_agg_call{entries[c].agg, entries[c].value};
        const int64_t mg = std::max<int64_t>(1, std::min<int64_t>(nrows, rdf_groupby_multi_capacity((int32_t)nc)));
        std::vector<std::shared_ptr<Array>> num(nk), offs(nk), data(nk), os(nc), oc(nc);
        std::vector<rdf_out> vk(nk), vo(nk), vd(nk), vs(nc), vcn(nc);
        std::vector<rdf_key_out> ko(nk);
        for (size_t k = 0; k < nk; ++k) {
            if (kcs[k]->data_type() == DataType::Utf8) {
                offs[k] = Array::make_out(DataType::Int32, mg + 3, true, false);
                data[k] = Array::make_out(DataType::UInt8, key_bytes[k] + 8, false, false);
                vo[k] = offs[k]->out_view(mg + 3);
                vd[k] = data[k]->out_view(key_bytes[k] + 8);
                ko[k] = rdf_key_out{nullptr, &vo[k], &vd[k]};
            } else {
                num[k] = Array::make_out(kcs[k]->data_type(), mg + 2, key_nulls[k], false);
                vk[k] = num[k]->out_view(mg + 2);
                ko[k] = rdf_key_out{&vk[k], nullptr, nullptr};
            }
        }
        for (size_t c = 0; c < nc; ++c) {
            const bool extremum = entries[c].agg == RDF_AGG_MIN || entries[c].agg == RDF_AGG_MAX;
            os[c] = Array::make_out(entries[c].sdt, mg + 2, extremum && entries[c].val_nulls, false);
            oc[c] = Array::make_out(DataType::Int64, mg + 2, false, false);
            vs[c] = os[c]->out_view(mg + 2);
            vcn[c] = oc[c]->out_view(mg + 2);
        }
        int64_t groups = 0;
        const rdf_status st = rdf_groupby_multi(sk.keys.data(), (int32_t)nk, vptr.data(), (int32_t)vcols.size(), (int64_t)nch, calls.data(), (int32_t)nc, mg,
                                                ko.data(), vs.data(), vcn.data(), nullptr, &groups);
        if (st == RDF_MEMORY_ERROR && mg < nrows) return false;   // more groups than the one-pass route holds
        check(st);
        std::vector<ArrayRef> ok(nk);
        for (size_t k = 0; k < nk; ++k) {
            if (num[k]) { num[k]->length = vk[k].length; num[k]->null_count = vk[k].null_count; ok[k] = num[k]; continue; }
            offs[k]->length = groups + 1;
            data[k]->length = vd[k].length;
            const std::vector<int32_t> o = offs[k]->values_to_host<int32_t>();
            const std::vector<uint8_t> bytes = data[k]->values_to_host<uint8_t>();
            offs[k]->length = groups;
            const std::vector<bool> valid = offs[k]->valid_to_host();
            std::vector<std::string> rows((size_t)groups);
            for (int64_t g = 0; g < groups; ++g) rows[(size_t)g].assign((const char*)bytes.data() + o[(size_t)g], (size_t)(o[(size_t)g + 1] - o[(size_t)g]));
            auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(rows)));
            if (vo[k].null_count > 0) {
                const auto bits = pack_bits(valid);
                a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
                check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
                a->null_count = vo[k].null_count;
            }
            ok[k] = a;
        }
        std::vector<Column> gc;
        std::vector<DataFrame::SortCriteria> order;
        for (size_t k = 0; k < nk; ++k) {
            gc.push_back(Column::from_arrays({ok[k]}, Field{"k" + std::to_string(k), kcs[k]->data_type(), true}));
            order.push_back(DataFrame::SortCriteria{"k" + std::to_string(k), false, false});
        }
        for (size_t c = 0; c < nc; ++c) {
            os[c]->length = oc[c]->length = vs[c].length;
            os[c]->null_count = vs[c].null_count;
            gc.push_back(Column::from_arrays({os[c]}, Field{"s" + std::to_string(c), entries[c].sdt, true}));
            gc.push_back(Column::from_arrays({oc[c]}, Field{"c" + std::to_string(c), DataType::Int64, false}));
        }
        const DataFrame g = DataFrame::from_columns(gc).sort(order);   // the one sort every column of the step shares
        std::vector<Column> cols;
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) {
                if (!hashed(a.function)) { append_sorted_aggregate(f, t.names, a.function, c, cols); continue; }
                if (cols.empty())
                    for (size_t k = 0; k < nk; ++k) cols.push_back(Column::from_arrays(g.column_by_name("k" + std::to_string(k)).data().chunks(), Field{t.names[k], kcs[k]->data_type(), true}));
                const int32_t agg = a.function == AF::Min ? RDF_AGG_MIN : a.function == AF::Max ? RDF_AGG_MAX : a.function == AF::Count ? RDF_AGG_COUNT : RDF_AGG_SUM;
                const int e = entry_of(agg, c);
                append_aggregate_column(a.function, c, entries[(size_t)e].vdt, entries[(size_t)e].sdt, g.column_by_name("s" + std::to_string(e)).data().chunks(),
                                        g.column_by_name("c" + std::to_string(e)).data().chunks(), cols);
            }
        out_cols = std::move(cols);
        return true;
    }

    // GroupAggregate whose grouping columns include Utf8 ones: one rdf_groupby_agg_keys per aggregation (the text keys are
    // dictionary-encoded on the device, the codes grouped next to the integer keys, the dictionary taken by the result's code
    // column); results ordered by the grouping columns — text in byte order, the NULL group last.
    static DataFrame group_aggregate_text(const DataFrame& f, const plan::Transformation& t) {
        using AF = plan::AggregateFunction;
        std::vector<const Column*> kcs;
        for (auto& n : t.names) {
            kcs.push_back(&f.column_by_name(n));
            if (!is_integer(kcs.back()->data_type()) && kcs.back()->data_type() != DataType::Utf8)
                throw DataFrameError(DataFrameError::ComputeError, "GroupAggregate: the grouping columns must be integer or Utf8 columns");
        }
        const size_t nk = kcs.size(), nch = kcs[0]->data().num_chunks();
        const int64_t nrows = (int64_t)f.num_rows();
        const bool on_host = f.numeric_columns_on_host();
        std::vector<DataFrame::SortCriteria> crit;
        for (auto& n : t.names) crit.push_back(DataFrame::SortCriteria{n, false, false});
        const DataFrame::SortKeys sk = f.sort_keys(crit, on_host);
        std::vector<bool> key_nulls(nk, false);
        std::vector<int64_t> key_bytes(nk, 0);
        for (size_t k = 0; k < nk; ++k) {
            for (auto& a : kcs[k]->data().chunks()) if (a->validity != nullptr) key_nulls[k] = true;
            for (auto& u : sk.txt[k]) key_bytes[k] += u.data.length;   // the key column's input bytes always suffice
        }
        std::vector<Column> out_cols;
        if (group_aggregate_multi(f, t, kcs, on_host, out_cols)) return DataFrame::from_columns(out_cols);   // two or more hash aggregations: one call, one sort
        std::vector<MomentCalls> moment_calls;
        auto one = [&](AF fn, const std::string& col) {
            if (fn == AF::CountDistinct || fn == AF::First || fn == AF::Last) { append_sorted_aggregate(f, t.names, fn, col, out_cols); return; }
            if (moment_function(fn)) { append_moment_aggregate(f, t, fn, col, moment_calls, out_cols); return; }
            if (fn != AF::Sum && fn != AF::Count && fn != AF::Avg && fn != AF::Min && fn != AF::Max) throw DataFrameError(DataFrameError::ComputeError, "Aggregation not yet supported");
            const Column& vc = f.column_by_name(col);
            const DataType vdt = vc.data_type();
            if (!(is_integer(vdt) || is_float(vdt))) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column must be numeric");
            std::vector<rdf_array> vals;
            bool val_nulls = false;
            for (auto& a : vc.data().chunks()) { vals.push_back(a->view()); val_nulls |= a->validity != nullptr; }
            const int32_t agg = fn == AF::Min ? RDF_AGG_MIN : fn == AF::Max ? RDF_AGG_MAX : RDF_AGG_SUM;
            const bool extremum = agg != RDF_AGG_SUM;
            const DataType sdt = is_float(vdt) ? DataType::Float64 : (extremum && vdt == DataType::UInt64) ? DataType::UInt64 : DataType::Int64;
            int64_t mg = std::max<int64_t>(1, std::min<int64_t>(nrows, (int64_t)1 << 20));
            std::vector<ArrayRef> ok(nk);
            std::shared_ptr<Array> os, oc;
            for (;;) {   // the number of groups is not known in advance: grow the promise until it holds
                std::vector<std::shared_ptr<Array>> num(nk), offs(nk), data(nk);
                std::vector<rdf_out> vk(nk), vo(nk), vd(nk);
                std::vector<rdf_key_out> ko(nk);
                for (size_t k = 0; k < nk; ++k) {
                    if (kcs[k]->data_type() == DataType::Utf8) {
                        offs[k] = Array::make_out(DataType::Int32, mg + 3, true, on_host);
                        data[k] = Array::make_out(DataType::UInt8, key_bytes[k] + 8, false, on_host);
                        vo[k] = offs[k]->out_view(mg + 3);
                        vd[k] = data[k]->out_view(key_bytes[k] + 8);
                        ko[k] = rdf_key_out{nullptr, &vo[k], &vd[k]};
                    } else {
                        num[k] = Array::make_out(kcs[k]->data_type(), mg + 2, key_nulls[k], on_host);
                        vk[k] = num[k]->out_view(mg + 2);
                        ko[k] = rdf_key_out{&vk[k], nullptr, nullptr};
                    }
                }
                os = Array::make_out(sdt, mg + 2, extremum && val_nulls, on_host);
                oc = Array::make_out(DataType::Int64, mg + 2, false, on_host);
                rdf_out vs = os->out_view(mg + 2), vcn = oc->out_view(mg + 2);
                const rdf_status st = rdf_groupby_agg_keys(sk.keys.data(), (int32_t)nk, vals.data(), (int64_t)nch, agg, mg, ko.data(), &vs, &vcn);
                if (st == RDF_MEMORY_ERROR && mg < nrows) { mg = std::min<int64_t>(nrows, mg * 16); continue; }
                check(st);
                const int64_t groups = vcn.length;
                for (size_t k = 0; k < nk; ++k) {
                    if (num[k]) { num[k]->length = vk[k].length; num[k]->null_count = vk[k].null_count; ok[k] = num[k]; continue; }
                    offs[k]->length = groups + 1;
                    data[k]->length = vd[k].length;
                    const std::vector<int32_t> o = offs[k]->values_to_host<int32_t>();
                    const std::vector<uint8_t> bytes = data[k]->values_to_host<uint8_t>();
                    offs[k]->length = groups;
                    const std::vector<bool> valid = offs[k]->valid_to_host();
                    std::vector<std::string> rows((size_t)groups);
                    for (int64_t g = 0; g < groups; ++g) rows[(size_t)g].assign((const char*)bytes.data() + o[(size_t)g], (size_t)(o[(size_t)g + 1] - o[(size_t)g]));
                    auto a = std::const_pointer_cast<Array>(Array::from_strings(std::move(rows)));
                    if (vo[k].null_count > 0) {
                        const auto bits = pack_bits(valid);
                        a->validity = std::make_shared<DeviceBuffer>((int64_t)bits.size());
                        check(rdf_copy_h2d(a->validity->data(), bits.data(), (int64_t)bits.size()));
                        a->null_count = vo[k].null_count;
                    }
                    ok[k] = a;
                }
                os->length = oc->length = vs.length;
                os->null_count = vs.null_count;
                break;
            }
            std::vector<Column> gc;
            std::vector<DataFrame::SortCriteria> order;
            for (size_t k = 0; k < nk; ++k) {
                gc.push_back(Column::from_arrays({ok[k]}, Field{"k" + std::to_string(k), kcs[k]->data_type(), true}));
                order.push_back(DataFrame::SortCriteria{"k" + std::to_string(k), false, false});
            }
            gc.push_back(Column::from_arrays({os}, Field{"s", sdt, true}));
            gc.push_back(Column::from_arrays({oc}, Field{"c", DataType::Int64, false}));
            DataFrame g = DataFrame::from_columns(gc).sort(order);
            if (out_cols.empty())
                for (size_t k = 0; k < nk; ++k) out_cols.push_back(Column::from_arrays(g.column_by_name("k" + std::to_string(k)).data().chunks(), Field{t.names[k], kcs[k]->data_type(), true}));
            append_aggregate_column(fn, col, vdt, sdt, g.column_by_name("s").data().chunks(), g.column_by_name("c").data().chunks(), out_cols);
        };
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) one(a.function, c);
        if (out_cols.empty()) throw DataFrameError(DataFrameError::ComputeError, "GroupAggregate without aggregations");
        return DataFrame::from_columns(out_cols);
    }

    void step_group_aggregate(const plan::Transformation& t) {
        using AF = plan::AggregateFunction;
        if (fused_dense_group_aggregate(t)) return;   // small dense key domain(s): filter + expressions + grouping in one pass
        DataFrame f = flush();   // lazy columns materialised, pending filters applied
        const size_t nk = t.names.size();
        if (nk < 1 || nk > RDF_MAX_GROUP_KEYS) throw DataFrameError(DataFrameError::ComputeError, "GroupAggregate: 1.." + std::to_string(RDF_MAX_GROUP_KEYS) + " grouping columns");
        std::vector<const Column*> kcs;
        for (auto& n : t.names) {
            kcs.push_back(&f.column_by_name(n));
            if (!is_integer(kcs.back()->data_type())) throw DataFrameError(DataFrameError::ComputeError, "GroupAggregate: the grouping columns must be integer columns");
        }
        const size_t nch = kcs[0]->data().num_chunks();
        std::vector<rdf_array> keys;          // [k * nch + i]
        std::vector<bool> key_nulls(nk, false);
        for (size_t k = 0; k < nk; ++k)
            for (auto& a : kcs[k]->data().chunks()) { keys.push_back(a->view()); if (a->validity != nullptr) key_nulls[k] = true; }
        const int64_t nrows = (int64_t)f.num_rows();
        std::vector<Column> out_cols;
        if (nk == 1 && dense_group_aggregate(f, *kcs[0], t, out_cols)) { reset(DataFrame::from_columns(out_cols)); return; }
        if (group_aggregate_multi(f, t, kcs, f.is_host(), out_cols)) { reset(DataFrame::from_columns(out_cols)); return; }   // two or more hash aggregations: one call, one sort
        // Sparse or NULL-holding keys: one rdf_groupby_agg per aggregation (hash GROUP BY; several grouping columns are
        // range-compressed into one 64-bit key on the device), results ordered by the grouping columns
        std::vector<MomentCalls> moment_calls;
        auto one = [&](AF fn, const std::string& col) {
            if (fn == AF::CountDistinct || fn == AF::First || fn == AF::Last) { append_sorted_aggregate(f, t.names, fn, col, out_cols); return; }
            if (moment_function(fn)) { append_moment_aggregate(f, t, fn, col, moment_calls, out_cols); return; }
            if (fn != AF::Sum && fn != AF::Count && fn != AF::Avg && fn != AF::Min && fn != AF::Max) throw DataFrameError(DataFrameError::ComputeError, "Aggregation not yet supported");
            const Column& vc = f.column_by_name(col);
            const DataType vdt = vc.data_type();
            if (!(is_integer(vdt) || is_float(vdt))) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column must be numeric");
            std::vector<rdf_array> vals;
            bool val_nulls = false;
            for (auto& a : vc.data().chunks()) { vals.push_back(a->view()); val_nulls |= a->validity != nullptr; }
            const int32_t agg = fn == AF::Min ? RDF_AGG_MIN : fn == AF::Max ? RDF_AGG_MAX : RDF_AGG_SUM;
            const bool extremum = agg != RDF_AGG_SUM;
            const DataType sdt = is_float(vdt) ? DataType::Float64 : (extremum && vdt == DataType::UInt64) ? DataType::UInt64 : DataType::Int64;
            int64_t mg = std::max<int64_t>(1, std::min<int64_t>(nrows, (int64_t)1 << 20));
            std::vector<std::shared_ptr<Array>> ok(nk);
            std::shared_ptr<Array> os, oc;
            for (;;) {   // the number of groups is not known in advance: grow the promise until it holds
                std::vector<rdf_out> vk(nk);
                const bool on_host = f.is_host();      // host-resident batches: the library streams them, the groups come back to the host
                for (size_t k = 0; k < nk; ++k) { ok[k] = Array::make_out(kcs[k]->data_type(), mg + 2, key_nulls[k], on_host); vk[k] = ok[k]->out_view(mg + 2); }
                os = Array::make_out(sdt, mg + 2, extremum && val_nulls, on_host);
                oc = Array::make_out(DataType::Int64, mg + 2, false, on_host);
                rdf_out vs = os->out_view(mg + 2), vcn = oc->out_view(mg + 2);
                const rdf_status st = rdf_groupby_agg(keys.data(), (int32_t)nk, vals.data(), (int64_t)nch, agg, mg, vk.data(), &vs, &vcn);
                if (st == RDF_MEMORY_ERROR && mg < nrows) { mg = std::min<int64_t>(nrows, mg * 16); continue; }
                check(st);
                for (size_t k = 0; k < nk; ++k) { ok[k]->length = vk[k].length; ok[k]->null_count = vk[k].null_count; }
                os->length = oc->length = vs.length;
                os->null_count = vs.null_count;
                break;
            }
            std::vector<Column> gc;
            std::vector<DataFrame::SortCriteria> order;
            for (size_t k = 0; k < nk; ++k) {
                gc.push_back(Column::from_arrays({ok[k]}, Field{"k" + std::to_string(k), kcs[k]->data_type(), true}));
                order.push_back(DataFrame::SortCriteria{"k" + std::to_string(k), false, false});
            }
            gc.push_back(Column::from_arrays({os}, Field{"s", sdt, true}));
            gc.push_back(Column::from_arrays({oc}, Field{"c", DataType::Int64, false}));
            DataFrame g = DataFrame::from_columns(gc).sort(order);
            if (out_cols.empty())
                for (size_t k = 0; k < nk; ++k) out_cols.push_back(Column::from_arrays(g.column_by_name("k" + std::to_string(k)).data().chunks(), Field{t.names[k], kcs[k]->data_type(), true}));
            append_aggregate_column(fn, col, vdt, sdt, g.column_by_name("s").data().chunks(), g.column_by_name("c").data().chunks(), out_cols);
        };
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) one(a.function, c);
        if (out_cols.empty()) throw DataFrameError(DataFrameError::ComputeError, "GroupAggregate without aggregations");
        reset(DataFrame::from_columns(out_cols));
    }

    // GroupAggregate over a SMALL DENSE key domain (dictionary codes, flags: TPC-H Q1's returnflag x linestatus): the pending
    // filter, the lazy value expressions, the grouping and every aggregation of the step in ONE pass over the rows through
    // rdf_group_pipeline (group id = mixed-radix number of the keys' offsets from their minima), instead of materialising the
    // computed columns and running one hash GROUP BY per aggregation.  Same output as the hash path: groups in ascending key
    // order, the NULL key (single grouping column only) last.  -> false when the shape does not fit the dense kernel
    // (RDF_MAX_GROUP_SLOTS / RDF_MAX_GROUP_VALUES, NULLs in one of several grouping columns, a non-integer key).
    struct DenseKey { std::string column, out_name; DataType dtype; };               // `column`: its name in `frame`
    struct DenseVal { plan::AggregateFunction fn; std::string name; DataType dtype; ExprRef e; };
    static bool dense_groups(const DataFrame& frame, const std::vector<DenseKey>& keys, const ExprRef& filter, const std::vector<DenseVal>& vals,
                             std::vector<Column>& out_cols) {
        using AF = plan::AggregateFunction;
        if (keys.empty() || vals.empty()) return false;
        // the dense kernel folds sums and counts; per-group Min / Max go through the hash path (rdf_groupby_agg)
        for (auto& v : vals) if (v.fn != AF::Sum && v.fn != AF::Count && v.fn != AF::Avg) return false;
        std::vector<int64_t> kmin(keys.size()), dom(keys.size());
        uint64_t total = 1;
        for (size_t i = 0; i < keys.size(); ++i) {
            if (!is_integer(keys[i].dtype)) return false;
            const Column& kc = frame.column_by_name(keys[i].column);
            const std::vector<rdf_array> kv = kc.data().views();
            if (keys.size() > 1) for (auto& a : kv) if (a.validity && a.null_count != 0) return false;   // NULLs would need one extra code per column
            unsigned char lo[8] = {0}, hi[8] = {0};
            int32_t some_lo = 0, some_hi = 0;
            check(rdf_min(kv.data(), (int64_t)kv.size(), lo, &some_lo));
            check(rdf_max(kv.data(), (int64_t)kv.size(), hi, &some_hi));
            if (!some_lo || !some_hi) return false;   // no non-NULL key at all
            auto as_i64 = [&](const unsigned char* p, bool& ok) -> int64_t {
                ok = true;
                switch (keys[i].dtype) {
                    case DataType::Int8: { int8_t v; std::memcpy(&v, p, 1); return v; }
                    case DataType::Int16: { int16_t v; std::memcpy(&v, p, 2); return v; }
                    case DataType::Int32: { int32_t v; std::memcpy(&v, p, 4); return v; }
                    case DataType::Int64: { int64_t v; std::memcpy(&v, p, 8); return v; }
                    case DataType::UInt8: { uint8_t v; std::memcpy(&v, p, 1); return v; }
                    case DataType::UInt16: { uint16_t v; std::memcpy(&v, p, 2); return v; }
                    case DataType::UInt32: { uint32_t v; std::memcpy(&v, p, 4); return v; }
                    default: { uint64_t v; std::memcpy(&v, p, 8); ok = v <= (uint64_t)INT64_MAX; return (int64_t)v; }
                }
            };
            bool ok_lo = false, ok_hi = false;
            const int64_t mn = as_i64(lo, ok_lo), mx = as_i64(hi, ok_hi);
            if (!ok_lo || !ok_hi || (uint64_t)mx - (uint64_t)mn >= (uint64_t)RDF_MAX_GROUP_SLOTS) return false;
            kmin[i] = mn;
            dom[i] = mx - mn + 1;
            total *= (uint64_t)dom[i];
            if (total > (uint64_t)RDF_MAX_GROUP_SLOTS) return false;
        }
        // the distinct value expressions of the step (Sum / Count / Avg of one column share its per-group sum and count)
        std::vector<std::string> vnames;
        std::vector<ExprRef> vexprs;
        for (auto& v : vals) {
            if (!(is_integer(v.dtype) || is_float(v.dtype))) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column must be numeric");
            if (std::find(vnames.begin(), vnames.end(), v.name) == vnames.end()) { vnames.push_back(v.name); vexprs.push_back(v.e); }
        }
        if (vnames.size() > (size_t)RDF_MAX_GROUP_VALUES || (size_t)(total + 1) * vnames.size() > (size_t)RDF_MAX_GROUP_SLOTS) return false;
        Lowered low;
        const int filter_root = filter ? low.add(filter) : -1;
        ExprRef gid;
        for (size_t i = 0; i < keys.size(); ++i) {
            ExprRef d = Expr::make(RDF_OP_SUB, Expr::make(RDF_OP_CAST, Expr::col(keys[i].column), nullptr, RDF_I64), Expr::literal(Scalar((int64_t)kmin[i]), RDF_I64));
            gid = i == 0 ? d : Expr::make(RDF_OP_ADD, Expr::make(RDF_OP_MUL, gid, Expr::literal(Scalar((int64_t)dom[i]), RDF_I64)), d);
        }
        const int group_root = low.add(gid);
        int32_t value_roots[RDF_MAX_GROUP_VALUES] = {0};
        for (size_t v = 0; v < vexprs.size(); ++v) value_roots[v] = low.add(vexprs[v]);
        std::vector<rdf_array> cols;
        for (auto& cn : low.columns) for (auto& a : frame.column_by_name(cn).data().chunks()) cols.push_back(a->view());
        const size_t S = (size_t)total + 1;
        std::vector<rdf_group_result> res(S * vnames.size());
        std::vector<int64_t> rows(S, 0);
        check(rdf_group_pipeline(low.nodes.data(), (int32_t)low.nodes.size(), filter_root, group_root, (int32_t)total, value_roots, (int32_t)vnames.size(),
                                 cols.data(), (int32_t)low.columns.size(), (int64_t)frame.num_chunks(), res.data(), rows.data()));
        // groups that hold rows, ascending (key 1, key 2, ..) = ascending slot, the NULL key (slot `total`) last
        std::vector<size_t> slots;
        for (size_t g = 0; g < S; ++g) if (rows[g] > 0) slots.push_back(g);
        const bool null_group = !slots.empty() && slots.back() == (size_t)total;
        for (size_t i = 0; i < keys.size(); ++i) {
            uint64_t below = 1;   // product of the domains of the keys after i
            for (size_t j = i + 1; j < keys.size(); ++j) below *= (uint64_t)dom[j];
            std::vector<int64_t> kvv;
            std::vector<bool> kvalid;
            for (size_t g : slots) {
                const bool isnull = g == (size_t)total;
                kvv.push_back(isnull ? 0 : kmin[i] + (int64_t)(((uint64_t)g / below) % (uint64_t)dom[i]));
                kvalid.push_back(!isnull);
            }
            const ArrayRef k64 = Array::from_vec<int64_t>(kvv, null_group ? &kvalid : nullptr);
            out_cols.push_back(Column::from_arrays(keys[i].dtype == DataType::Int64 ? std::vector<ArrayRef>{k64} : ScalarFunctions::cast({k64}, keys[i].dtype),
                                                   Field{keys[i].out_name, keys[i].dtype, true}));
        }
        for (auto& val : vals) {
            const size_t v = (size_t)(std::find(vnames.begin(), vnames.end(), val.name) - vnames.begin());
            const DataType vdt = val.dtype;
            std::vector<double> fs;
            std::vector<int64_t> is, cs;
            for (size_t g : slots) { const rdf_group_result& r = res[v * S + g]; fs.push_back(r.sum_f64); is.push_back(r.sum_i64); cs.push_back(r.count); }
            if (val.fn == AF::Sum) {
                const ArrayRef sums = is_float(vdt) ? Array::from_vec<double>(fs) : Array::from_vec<int64_t>(is);
                const DataType sdt = is_float(vdt) ? DataType::Float64 : DataType::Int64;
                out_cols.push_back(Column::from_arrays(sdt == vdt ? std::vector<ArrayRef>{sums} : ScalarFunctions::cast({sums}, vdt), Field{"sum(" + val.name + ")", vdt, true}));
            } else if (val.fn == AF::Count) {
                out_cols.push_back(Column::from_arrays(ScalarFunctions::cast({Array::from_vec<int64_t>(cs)}, DataType::UInt32), Field{"count(" + val.name + ")", DataType::UInt32, true}));
            } else {
                std::vector<double> m(slots.size());
                std::vector<bool> valid(slots.size());
                for (size_t r = 0; r < slots.size(); ++r) { valid[r] = cs[r] > 0; m[r] = cs[r] > 0 ? (is_float(vdt) ? fs[r] : (double)is[r]) / (double)cs[r] : 0.0; }
                out_cols.push_back(Column::from_arrays({Array::from_vec(m, &valid)}, Field{"avg(" + val.name + ")", DataType::Float64, true}));
            }
        }
        return true;
    }
    // the step as it stands in the lazy state: grouping columns that are columns of base_, the pending filter, lazy value expressions
    bool fused_dense_group_aggregate(const plan::Transformation& t) {
        if (t.names.empty() || t.names.size() > 4) return false;
        std::vector<DenseKey> keys;
        for (auto& n : t.names) {
            Entry* e = find(n);
            if (!e || e->def) return false;   // unknown (the caller reports it) or computed: not a column of base_
            keys.push_back(DenseKey{e->source, n, e->dtype});
        }
        std::vector<DenseVal> vals;
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) {
                Entry* e = find(c);
                if (!e) return false;
                vals.push_back(DenseVal{a.function, c, e->dtype, ref(c)});
            }
        std::vector<Column> out_cols;
        if (!dense_groups(base_, keys, pending_, vals, out_cols)) return false;
        reset(DataFrame::from_columns(out_cols));
        return true;
    }
    static bool dense_group_aggregate(const DataFrame& f, const Column& kc, const plan::Transformation& t, std::vector<Column>& out_cols) {
        std::vector<DenseVal> vals;
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) vals.push_back(DenseVal{a.function, c, f.column_by_name(c).data_type(), Expr::col(c)});
        return dense_groups(f, {DenseKey{kc.name(), kc.name(), kc.data_type()}}, nullptr, vals, out_cols);
    }

    void step_aggregate(const plan::Transformation& t) {
        if (!t.names.empty()) { step_group_aggregate(t); return; }
        struct Want { plan::AggregateFunction fn; std::string col; DataType dt; ExprRef e; };
        std::vector<Want> wants;
        for (auto& a : t.aggregations)
            for (auto& c : a.columns) {
                Entry* e = find(c);
                if (!e) throw DataFrameError(DataFrameError::ComputeError, "Aggregating column \"" + c + "\" does not exist");
                wants.push_back(Want{a.function, c, e->dtype, a.function == plan::AggregateFunction::Avg && !is_float(e->dtype)
                                                                   ? Expr::make(RDF_OP_CAST, ref(c), nullptr, RDF_F64) : ref(c)});
            }
        std::vector<Column> out_cols;
        for (size_t b = 0; b < wants.size(); b += RDF_MAX_VALUES) {
            const size_t n = std::min<size_t>(RDF_MAX_VALUES, wants.size() - b);
            Lowered low;
            rdf_program prog;
            std::memset(&prog, 0, sizeof prog);
            prog.filter_root = pending_ ? low.add(pending_) : -1;
            for (size_t k = 0; k < n; ++k) prog.value_roots[k] = low.add(wants[b + k].e);
            prog.nvalues = (int32_t)n;
            prog.sink = RDF_SINK_AGG;
            prog.nodes = low.nodes.data();
            prog.nnodes = (int32_t)low.nodes.size();
            std::vector<rdf_array> cols;
            for (auto& cn : low.columns) for (auto& a : base_.column_by_name(cn).data().chunks()) cols.push_back(a->view());
            rdf_agg_result res[RDF_MAX_VALUES];
            check(rdf_pipeline(&prog, cols.data(), (int32_t)low.columns.size(), (int64_t)base_.num_chunks(), nullptr, res));
            for (size_t k = 0; k < n; ++k) out_cols.push_back(agg_column(wants[b + k].fn, wants[b + k].col, wants[b + k].dt, res[k]));
        }
        reset(DataFrame::from_columns(out_cols));
    }
    // output naming / typing of Dataset::try_aggregate (src/expression.rs:114-221)
    static Column agg_column(plan::AggregateFunction fn, const std::string& col, DataType dt, const rdf_agg_result& r) {
        using AF = plan::AggregateFunction;
        const std::vector<bool> some{r.is_some != 0};
        auto mk = [&](const std::string& name, DataType t, double f, int64_t i, bool always) -> Column {
            const std::vector<bool>* valid = always ? nullptr : &some;
            ArrayRef a;
            switch (t) {
                case DataType::Float64: a = Array::from_vec(std::vector<double>{f}, valid); break;
                case DataType::Float32: a = Array::from_vec(std::vector<float>{(float)f}, valid); break;
                case DataType::Int64: a = Array::from_vec(std::vector<int64_t>{i}, valid); break;
                case DataType::UInt64: a = Array::from_vec(std::vector<uint64_t>{(uint64_t)i}, valid); break;
                case DataType::Int32: a = Array::from_vec(std::vector<int32_t>{(int32_t)i}, valid); break;
                case DataType::UInt32: a = Array::from_vec(std::vector<uint32_t>{(uint32_t)i}, valid); break;
                case DataType::Int16: a = Array::from_vec(std::vector<int16_t>{(int16_t)i}, valid); break;
                case DataType::UInt16: a = Array::from_vec(std::vector<uint16_t>{(uint16_t)i}, valid); break;
                case DataType::Int8: a = Array::from_vec(std::vector<int8_t>{(int8_t)i}, valid); break;
                default: a = Array::from_vec(std::vector<uint8_t>{(uint8_t)i}, valid); break;
            }
            return Column::from_arrays({a}, Field{name, t, true});
        };
        const bool fl = is_float(dt);
        switch (fn) {
            case AF::Sum: return mk("sum(" + col + ")", dt, r.sum_f64, r.sum_i64, true);
            case AF::Min: return mk("min(" + col + ")", dt, r.min_f64, r.min_i64, false);
            case AF::Max: return mk("max(" + col + ")", dt, r.max_f64, r.max_i64, false);
            case AF::Count:
                if (r.count > (int64_t)UINT32_MAX) throw DataFrameError(DataFrameError::ComputeError, "count does not fit the UInt32 the reference's schema declares");
                return mk("count(" + col + ")", DataType::UInt32, 0, r.count, true);
            case AF::Avg: return mk("avg(" + col + ")", DataType::Float64, r.count ? r.sum_f64 / (double)r.count : 0.0, 0, false);
            default: (void)fl; throw DataFrameError(DataFrameError::ComputeError, "Aggregation not yet supported");
        }
    }

    void reset(const DataFrame& f) {
        base_ = f;
        cols_.clear();
        pending_ = nullptr;
        for (auto& fld : f.schema().fields) cols_.push_back(Entry{fld.name, fld.data_type, nullptr, fld.name});
    }

    // materialise: every lazy column through a fused SINK_STORE pass, then
    // the pending predicate as ONE mask + ONE compaction of all columns.
    DataFrame flush() {
        const size_t nch = base_.num_chunks();
        std::vector<Column> out(cols_.size());
        std::vector<size_t> lazy;
        for (size_t i = 0; i < cols_.size(); ++i) {
            if (cols_[i].def) lazy.push_back(i);
            else out[i] = base_.column_by_name(cols_[i].source).renamed(cols_[i].name);
        }
        if (!lazy.empty() && base_.num_columns() == 0) throw DataFrameError(DataFrameError::ComputeError, "calculation on an empty frame");
        const auto counts = base_.num_columns() ? base_.column(0).data().chunk_counts() : std::vector<int64_t>{};
        // One pass per lazy column: a single-value program is what the two kernel catalogs (exact shapes, then tree
        // shapes with runtime operators) are keyed on — 0.6-0.7 of the HBM peak against 0.36-0.44 for a multi-value
        // pass on the general evaluator, which more than pays for re-reading a shared input column.
        constexpr size_t kValuesPerPass = 1;
        for (size_t b = 0; b < lazy.size(); b += kValuesPerPass) {
            const size_t n = std::min<size_t>(kValuesPerPass, lazy.size() - b);
            Lowered low;
            rdf_program prog;
            std::memset(&prog, 0, sizeof prog);
            prog.filter_root = -1;
            for (size_t k = 0; k < n; ++k) prog.value_roots[k] = low.add(cols_[lazy[b + k]].def);
            prog.nvalues = (int32_t)n;
            prog.sink = RDF_SINK_STORE;
            prog.nodes = low.nodes.data();
            prog.nnodes = (int32_t)low.nodes.size();
            std::vector<rdf_array> cv;
            for (auto& cn : low.columns) for (auto& a : base_.column_by_name(cn).data().chunks()) cv.push_back(a->view());
            std::vector<std::shared_ptr<Array>> outs;
            std::vector<rdf_out> ov;
            for (size_t k = 0; k < n; ++k)
                for (size_t i = 0; i < nch; ++i) { outs.push_back(Array::make_out(cols_[lazy[b + k]].dtype, counts[i], true, base_.is_host())); ov.push_back(outs.back()->out_view(counts[i])); }
            check(rdf_pipeline(&prog, cv.data(), (int32_t)low.columns.size(), (int64_t)nch, ov.data(), nullptr));
            for (size_t k = 0; k < n; ++k) {
                std::vector<ArrayRef> chunks;
                for (size_t i = 0; i < nch; ++i) {
                    auto& o = outs[k * nch + i];
                    o->length = ov[k * nch + i].length;
                    o->null_count = ov[k * nch + i].null_count;
                    if (o->null_count == 0) o->validity.reset();  // no nulls resulted: drop the bitmap like Arrow builders do
                    chunks.push_back(o);
                }
                out[lazy[b + k]] = Column::from_arrays(chunks, Field{cols_[lazy[b + k]].name, cols_[lazy[b + k]].dtype, true});
            }
        }
        DataFrame result = DataFrame::from_columns(out);
        if (pending_) {
            Lowered low;
            const int root = low.add(pending_);
            const Column mask = base_.run_predicate(low, root);
            result = result.filter_by_mask(mask);
        }
        reset(result);
        return result;
    }

    DataFrame base_;
    std::vector<Entry> cols_;
    ExprRef pending_;
};

// ------------------------------------------------------------------------------------------------
// LazyFrame (src/lazyframe.rs:15-315): a plan builder over an in-memory source frame

class LazyFrame {
  public:
    static LazyFrame read(const DataFrame& source) {
        LazyFrame f;
        f.source_ = std::make_shared<DataFrame>(source);
        f.output_.name = "source";
        for (auto& fld : source.schema().fields) f.output_.columns.push_back(plan::Column{fld.name, fld.data_type});
        return f;
    }
    // LazyFrame::read(Computation) (src/lazyframe.rs:25-38): the plan starts at a Reader; nothing is loaded until evaluate(),
    // which first runs plan::optimise over the unrolled plan — a Limit / Select next to a CSV read becomes the reader's
    // max_records / projection, so the rows and columns that are not wanted are never parsed, uploaded or computed on.
    static LazyFrame read(const plan::Computation& read_computation) {
        if (!read_computation.is_single(plan::Transformation::Read)) throw DataFrameError(DataFrameError::ComputeError, "LazyFrame::read expects a read computation");
        LazyFrame f;
        f.read_ = std::make_shared<plan::Computation>(read_computation);
        f.output_ = read_computation.output;
        return f;
    }
    std::optional<std::pair<size_t, plan::Column>> column(const std::string& name) const { return output_.get_column(name); }
    const plan::Dataset& output() const { return output_; }
    // Expression::unroll (src/expression.rs:516-553): newest computation first, the read (if the plan has one) last
    std::vector<plan::Computation> unroll() const {
        std::vector<plan::Computation> u(comps_.rbegin(), comps_.rend());
        if (read_) u.push_back(*read_);
        return u;
    }
    // the plan after plan::optimise to a fixed point (the reference's tests apply it twice to merge a Select and a Limit into the read)
    std::vector<plan::Computation> optimised() const {
        std::vector<plan::Computation> u = unroll();
        for (int pass = 0; pass < 4; ++pass) {
            std::vector<plan::Computation> o = plan::optimise(u);
            const bool same = o.size() == u.size();
            u = std::move(o);
            if (same && pass > 0) break;
        }
        return u;
    }

    LazyFrame with_column(const std::string& col_name, const plan::Function& function, const std::vector<std::string>& input_col_names,
                          std::optional<DataType> as_type = std::nullopt) const {  // :58-96
        auto ops = plan::calculate(output_, input_col_names, function, col_name, as_type);
        LazyFrame f = *this;
        for (auto& t : ops) {
            if (t.kind != plan::Transformation::Calculate) throw DataFrameError(DataFrameError::ComputeError, "can't create column from a non-calculation transformation");
            f.output_ = f.output_.append_column(t.calc.output);
        }
        f.push(ops, output_);
        return f;
    }
    LazyFrame with_column_renamed(const std::string& old_name, const std::string& new_name) const {  // :98-131
        auto c = output_.get_column(old_name);
        if (!c) return *this;
        LazyFrame f = *this;
        f.output_.columns[c->first].name = new_name;
        f.output_.name = "renamed_dataset";
        f.push({plan::Transformation::Calculate_(plan::Calculation{"rename", {c->second}, plan::Column{new_name, c->second.data_type}, plan::Function::Rename_()})}, output_);
        return f;
    }
    LazyFrame filter(const FilterRef& cond) const { LazyFrame f = *this; f.push({plan::Transformation::Filter_(cond)}, output_); return f; }
    LazyFrame limit(size_t n) const { LazyFrame f = *this; f.push({plan::Transformation::Limit_(n)}, output_); return f; }
    LazyFrame select(const std::vector<std::string>& names) const {
        LazyFrame f = *this;
        plan::Dataset d; d.name = output_.name;
        for (auto& c : output_.columns) for (auto& n : names) if (c.name == n) { d.columns.push_back(c); break; }
        f.output_ = d;
        f.push({plan::Transformation::Select_(names)}, output_);
        return f;
    }
    LazyFrame drop(const std::vector<std::string>& names) const {
        LazyFrame f = *this;
        plan::Dataset d; d.name = output_.name;
        for (auto& c : output_.columns) { bool x = false; for (auto& n : names) x |= c.name == n; if (!x) d.columns.push_back(c); }
        f.output_ = d;
        f.push({plan::Transformation::Drop_(names)}, output_);
        return f;
    }
    LazyFrame sort(const std::vector<std::string>& cols, const std::vector<bool>& descending) const {
        LazyFrame f = *this;
        f.push({plan::Transformation::Sort_(cols, descending)}, output_);
        return f;
    }
    // LazyFrame::join (:225-251) with Dataset::try_join's checks and output naming (src/expression.rs:223-285): both key
    // columns must exist and have the same type; a column name present on both sides comes out as "a.<name>" / "b.<name>".
    // Evaluation is the reference's (src/evaluation.rs:75-84): both sub-plans are evaluated, then DataFrame::join (the
    // index pairs come from rdf_equijoin_indices_multi, the columns from rdf_take); the joined frame is the new source.
    LazyFrame join(const LazyFrame& other, const DataFrame::JoinCriteria& jc) const {
        const plan::Dataset planned = plan::try_join(output_, other.output_, jc.criteria);
        const DataFrame j = evaluate().join(other.evaluate(), jc);
        std::vector<Column> cols;
        for (size_t k = 0; k < planned.columns.size(); ++k) cols.push_back(j.column(k).renamed(planned.columns[k].name));
        LazyFrame f = LazyFrame::read(DataFrame::from_columns(cols));
        f.output_.name = planned.name;
        return f;
    }
    LazyFrame aggregate(const std::vector<std::string>& groups, const std::vector<plan::Aggregation>& aggr) const {   // :285-309
        LazyFrame f = *this;
        f.output_ = plan::try_aggregate(output_, groups, aggr);
        f.push({plan::Transformation::GroupAggregate_(groups, aggr)}, output_);
        return f;
    }
    // LazyFrame::evaluate (:311-315): unroll (newest first) and hand to Evaluate
    DataFrame evaluate() const {
        if (!read_) {
            std::vector<plan::Computation> unrolled(comps_.rbegin(), comps_.rend());
            return Evaluate::evaluate(*source_, unrolled);
        }
        std::vector<plan::Computation> plan_ = optimised();
        if (plan_.empty() || !plan_.back().is_single(plan::Transformation::Read)) throw DataFrameError(DataFrameError::ComputeError, "optimised plan does not end in a read");
        const plan::Reader& r = plan_.back().transformations[0].reader;
        DataFrame source = r.source == plan::Reader::Csv ? DataFrame::from_csv(r.path, r.csv)
                         : r.source == plan::Reader::Arrow ? DataFrame::from_arrow(r.path)
                         : throw DataFrameError(DataFrameError::ComputeError, "only CSV and Arrow IPC sources are loaded here");
        plan_.pop_back();
        return Evaluate::evaluate(source, plan_);
    }

  private:
    // one Computation per pushed step: input = the dataset before it (what `this` planned), output = the dataset after it
    void push(std::vector<plan::Transformation> t, const plan::Dataset& before) {
        plan::Computation c;
        c.input = {before};
        c.transformations = std::move(t);
        c.output = output_;
        comps_.push_back(std::move(c));
    }
    std::shared_ptr<DataFrame> source_;
    std::shared_ptr<plan::Computation> read_;   // set when the plan starts at a Reader instead of a loaded frame
    plan::Dataset output_;
    std::vector<plan::Computation> comps_;  // oldest first
};

}  // namespace rdf
