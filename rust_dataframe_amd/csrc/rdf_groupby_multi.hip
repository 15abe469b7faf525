// rdf_groupby_multi.hip — hash GROUP BY with up to 8 aggregates folded into ONE table from one pass over the keys
// (rdf_groupby_multi; host side: rdf_capi_groupby_multi.inc, route and LDS layout: rdf_groupby_multi_plan.h).
//
// The key column is what rdf_groupby_agg's front makes of the grouping columns: one integer column, several columns packed
// into 64 bits, Utf8 columns as dictionary codes.  Behind it two routes end in the same table in HBM (GbmTable):
//   gbm_stream_kernel   gb2_stream_kernel widened to K accumulators: every block folds its rows into an LDS table of hashed
//                       keys — a row resolves its slot ONCE, then adds into the slot's K accumulators with LDS atomics — and
//                       merges its groups into the global table at the end.  Chosen while the promised groups fit the table.
//   gbm_table_kernel    any number of groups: rows go straight to the global table, insert-or-find and K global atomics.
// gbm_emit_kernel compacts the occupied entries to dense rows (the two set-aside groups last), gbm_finish_kernel turns the
// MIN / MAX images back into values and writes validity and null counts.
//
// Textually included at the end of rdf_groupby.hip (one translation unit): g2_hash / g2_unhash, kFree, mix64b, ord_bits /
// unord_bits, to_table_form, acc_apply and g2_load_raw are that file's.
#include "rdf_groupby_multi_plan.h"

namespace rdfk {

constexpr int kGbmBlock = 512;
static_assert(kGbmBlock == kGbmSub, "thread t holds row t of a sub-tile");

__device__ __forceinline__ int gbm_value_class(int dt) { return (dt == RDF_F32 || dt == RDF_F64) ? CLS_F64 : dt_is_signed(dt) ? CLS_SIGNED : CLS_UNSIGNED; }
__device__ __forceinline__ int gbm_first(const GbmArgs& a, int v) { return (int)((a.first_bits >> (4 * v)) & 15u); }
__device__ __forceinline__ int gbm_order_call(const GbmArgs& a, int i) { return (int)((a.order_bits >> (8 * i)) & 7u); }
__device__ __forceinline__ int gbm_call_op(uint32_t call_bits, int c) { return (int)((call_bits >> (4 * c)) & 3u); }
__device__ __forceinline__ int gbm_call_cls(uint32_t call_bits, int c) { return (int)((call_bits >> (4 * c + 2)) & 3u); }

// ------------------------------------------------------------------------------------------------
// rows of R consecutive sub-tiles: thread t holds row t of each.  Nothing here consumes a load.

template <int R, int NV>
struct GbmRaw {
    uint64_t key[R], val[R][NV];
    uint32_t kb[R], vb[R][NV];     // the validity BYTE holding the row's bit (0xFF: no bitmap)
    uint32_t bits[R];              // 3 bits per column (key first): bit position inside that byte
    uint32_t exists;
};

template <int R, int NV>
__device__ __forceinline__ void gbm_load(const GbmArgs& a, int64_t st, int tid, GbmRaw<R, NV>& r) {
    const int ksz = g2_dtype_size(a.key_dtype);
    r.exists = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int64_t sub = st + j;
        DevChunkCol kc = DevChunkCol{nullptr, nullptr, 0};
        int64_t r0 = 0, clen = 0, c = 0;
        if (sub < a.nsubs) {
            if (a.nchunks == 1) { kc = a.key0; r0 = sub * kGbmSub; clen = a.len0; }
            else {
                const ConstPtr<int64_t> sub_start = as_const<int64_t>(a.chunk_sub_start);
                c = find_chunk_tile(sub_start, a.nchunks, sub);
                r0 = (sub - sub_start[c]) * kGbmSub;
                clen = as_const<int64_t>(a.chunk_len)[c];
                kc = const_col(a.keys, c);
            }
        }
        const int64_t row = r0 + tid;
        const bool e = row < clen;
        r.exists |= (uint32_t)e << j;
        r.bits[j] = 0;
        r.key[j] = g2_load_raw(kc.values, ksz, kc.offset + row, e);
        r.kb[j] = 0xFFu;
        if (kc.validity) {
            const int64_t b = kc.offset + row;
            if (e) r.kb[j] = as_global<uint8_t>(kc.validity)[b >> 3];
            r.bits[j] |= (uint32_t)(b & 7);
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            r.val[j][v] = 0;
            r.vb[j][v] = 0xFFu;
            if (v >= a.nvalues) continue;
            DevChunkCol vc = DevChunkCol{nullptr, nullptr, 0};
            if (sub < a.nsubs) vc = a.nchunks == 1 ? a.val0[v] : const_col(a.values, (int64_t)v * a.nchunks + c);
            r.val[j][v] = g2_load_raw(vc.values, g2_dtype_size(a.value_dtype[v]), vc.offset + row, e);
            if (vc.validity) {
                const int64_t b = vc.offset + row;
                if (e) r.vb[j][v] = as_global<uint8_t>(vc.validity)[b >> 3];
                r.bits[j] |= (uint32_t)(b & 7) << (3 * (v + 1));
            }
        }
    }
}

// value of column v as the accumulators take it: f32 widened, integers sign- / zero-extended
__device__ __forceinline__ uint64_t gbm_native(int dt, uint64_t raw) {
    if (dt == RDF_F32) return d2u((double)__uint_as_float((uint32_t)raw));
    if (dt == RDF_F64) return raw;
    return normalize_int(dt, raw);
}

// the contributions of row j to entry e of the block table (32-bit counts) or the global table (64-bit counts)
template <int R, int NV, class CntT>
__device__ __forceinline__ void gbm_fold_row(const GbmArgs& a, const GbmRaw<R, NV>& r, int j, unsigned long long* acc, CntT* cnt, int64_t entries, int64_t e) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        if (v >= a.nvalues) continue;
        const bool vnull = ((r.vb[j][v] >> ((r.bits[j] >> (3 * (v + 1))) & 7)) & 1u) == 0;
        if (vnull) continue;
        const int dt = a.value_dtype[v];
        const int cls = gbm_value_class(dt);
        const uint64_t nv = gbm_native(dt, r.val[j][v]);
        const int i1 = gbm_first(a, v + 1);
        for (int i = gbm_first(a, v); i < i1; ++i) {
            const int c = gbm_order_call(a, i);
            const int op = gbm_call_op(a.call_bits, c);
            if (op != GBM_COUNT) {
                const uint64_t tf = to_table_form(op, cls, nv, false);
                if (op == AGG_SUM || tf != agg_identity(op)) acc_apply(&acc[(int64_t)c * entries + e], op, cls, tf);
            }
            atomicAdd(&cnt[(int64_t)c * entries + e], (CntT)1);
        }
    }
}

// insert-or-find a hashed key in the global table; -1: the table is full
__device__ __forceinline__ int64_t gbm_global_slot(const GbmTable& t, uint64_t hk) {
    const uint64_t mask = (uint64_t)t.capacity - 1;
    uint64_t s = mix64b(hk) & mask;
    int64_t probes = 0;
    for (;;) {
        unsigned long long old = t.keys[s];
        if (old == kFree) {
            old = atomicCAS(&t.keys[s], kFree, (unsigned long long)hk);
            if (old == kFree) { atomicAdd(&t.head[0], 1u); return (int64_t)s; }
        }
        if (old == hk) return (int64_t)s;
        s = (s + 1) & mask;
        if (++probes > t.capacity) return -1;
    }
}

// ------------------------------------------------------------------------------------------------
// route 1: columns -> per-block LDS table -> global table

struct GbmLds {
    unsigned long long* keys;   // [entries]
    unsigned long long* acc;    // [ncalls][entries]
    unsigned int*       rows;   // [entries]
    unsigned int*       cnt;    // [ncalls][entries]
};

template <int R, int NV>
__global__ __launch_bounds__(kGbmBlock, 4) void gbm_stream_kernel(const GbmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gbm_sm[];
    const int slots = a.slots, entries = slots + 2;
    GbmLds t;
    t.keys = (unsigned long long*)gbm_sm;
    t.acc = (unsigned long long*)(gbm_sm + a.off_acc);
    t.rows = (unsigned int*)(gbm_sm + a.off_rows);
    t.cnt = (unsigned int*)(gbm_sm + a.off_cnt);
    const int tid = threadIdx.x;
    for (int i = tid; i < entries; i += kGbmBlock) { t.keys[i] = kFree; t.rows[i] = 0; }
    for (int c = 0; c < a.ncalls; ++c) {
        const unsigned long long ident = agg_identity(gbm_call_op(a.call_bits, c));
        for (int i = tid; i < entries; i += kGbmBlock) { t.acc[c * entries + i] = ident; t.cnt[c * entries + i] = 0; }
    }
    __syncthreads();
    uint32_t err = 0;
    const int64_t stride = (int64_t)gridDim.x * R;
    int64_t st = (int64_t)blockIdx.x * R;
    auto fold = [&](const GbmRaw<R, NV>& raw) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (!((raw.exists >> j) & 1) || err) continue;   // (a block whose table overflowed stops folding)
            const bool knull = ((raw.kb[j] >> (raw.bits[j] & 7)) & 1u) == 0;
            const uint64_t hk = g2_hash(normalize_int(a.key_dtype, raw.key[j]));
            int e;
            if (knull) e = slots + 1;
            else if (hk == kFree) e = slots;
            else {
                uint32_t s = (uint32_t)(((uint64_t)(uint32_t)(hk >> 32) * (uint64_t)(uint32_t)slots) >> 32);
                int guard = 0;
                e = -1;
                for (;;) {
                    unsigned long long old = t.keys[s];
                    if (old == kFree) {
                        old = atomicCAS(&t.keys[s], kFree, (unsigned long long)hk);
                        if (old == kFree) old = hk;
                    }
                    if (old == hk) { e = (int)s; break; }
                    if (++s == (uint32_t)slots) s = 0;
                    if (++guard > slots) break;
                }
                if (e < 0) { err |= 8u; continue; }
            }
            atomicAdd(&t.rows[e], 1u);
            gbm_fold_row<R, NV>(a, raw, j, t.acc, t.cnt, entries, e);
        }
    };
    // The load pipeline of gb2_stream_kernel: the next batch's loads (keys and every value column) fly while this one is
    // folded; the two register sets rotate by unrolling, never by copying, and the prefetch is unconditional (past the end
    // the block's last batch is loaded again and never folded).
    const int64_t last_st = ((a.nsubs - 1) / R) * R;
    auto prefetch = [&](GbmRaw<R, NV>& dst, int64_t at) { gbm_load<R, NV>(a, at < a.nsubs ? at : last_st, tid, dst); };
    if (st < a.nsubs) {
        GbmRaw<R, NV> ra, rb;
        prefetch(ra, st);
        for (;;) {
            prefetch(rb, st + stride); fold(ra); st += stride; if (st >= a.nsubs) break;
            prefetch(ra, st + stride); fold(rb); st += stride; if (st >= a.nsubs) break;
        }
    }
    __syncthreads();
    // the block's groups -> the global table
    for (int i = tid; i < entries; i += kGbmBlock) {
        const unsigned long long hk = t.keys[i];
        const unsigned int rows = t.rows[i];
        if (i < slots ? hk == kFree : rows == 0) continue;
        const int64_t g = i < slots ? gbm_global_slot(a.t, hk) : a.t.capacity + (i - slots);
        if (g < 0) { err |= 4u; continue; }
        atomicAdd(&a.t.rows[g], (unsigned long long)rows);
        for (int c = 0; c < a.ncalls; ++c) {
            const unsigned int n = t.cnt[c * entries + i];
            if (!n) continue;   // (calls that count rows never count here)
            const int op = gbm_call_op(a.call_bits, c);
            if (op != GBM_COUNT) acc_apply(&a.t.acc[(int64_t)c * a.t.entries + g], op, gbm_call_cls(a.call_bits, c), t.acc[c * entries + i]);
            atomicAdd(&a.t.cnt[(int64_t)c * a.t.entries + g], (unsigned long long)n);
        }
    }
    if (err) atomicOr(&a.t.head[1], err);
}

// ------------------------------------------------------------------------------------------------
// route 2: rows -> global table

template <int R, int NV>
__global__ __launch_bounds__(kGbmBlock, 4) void gbm_table_kernel(const GbmArgs a) {
    const int tid = threadIdx.x;
    uint32_t err = 0;
    for (int64_t st = (int64_t)blockIdx.x * R; st < a.nsubs; st += (int64_t)gridDim.x * R) {
        GbmRaw<R, NV> raw;
        gbm_load<R, NV>(a, st, tid, raw);
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (!((raw.exists >> j) & 1)) continue;
            const bool knull = ((raw.kb[j] >> (raw.bits[j] & 7)) & 1u) == 0;
            const uint64_t hk = g2_hash(normalize_int(a.key_dtype, raw.key[j]));
            const int64_t g = knull ? a.t.capacity + 1 : hk == kFree ? a.t.capacity : gbm_global_slot(a.t, hk);
            if (g < 0) { err |= 4u; continue; }
            atomicAdd(&a.t.rows[g], 1ull);
            gbm_fold_row<R, NV>(a, raw, j, a.t.acc, a.t.cnt, a.t.entries, g);
        }
    }
    if (err) atomicOr(&a.t.head[1], err);
}

// ------------------------------------------------------------------------------------------------
// occupied entries -> dense rows (keys un-hashed, raw accumulators, counts); the two set-aside groups last

__global__ __launch_bounds__(kBlock) void gbm_emit_kernel(const GbmEmitArgs a) {
    const int64_t cap = a.t.capacity;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < a.t.entries; s += (int64_t)gridDim.x * kBlock) {
        const unsigned long long hk = a.t.keys[s], rows = a.t.rows[s];
        int64_t idx;
        uint64_t key;
        if (s < cap) {
            if (hk == kFree) continue;
            idx = (int64_t)atomicAdd(&a.t.head[2], 1u);
            key = g2_unhash(hk);
        } else {
            if (rows == 0) continue;
            idx = a.ng_main + (s == cap + 1 && a.t.rows[cap] != 0 ? 1 : 0);
            key = s == cap ? g2_unhash(kFree) : 0ull;
        }
        if (idx >= a.cap_out) continue;   // (the host has compared the group count with the buffers before this launch)
        switch (a.key_dtype) {
            case RDF_I32: case RDF_U32: ((uint32_t*)a.out_keys)[idx] = (uint32_t)key; break;
            case RDF_I16: case RDF_U16: ((uint16_t*)a.out_keys)[idx] = (uint16_t)key; break;
            case RDF_I8: case RDF_U8: ((uint8_t*)a.out_keys)[idx] = (uint8_t)key; break;
            default: ((uint64_t*)a.out_keys)[idx] = key; break;
        }
        if (s != cap + 1) atomicOr(a.out_keys_validity + (idx >> 5), 1u << (idx & 31));
        a.out_rows[idx] = (int64_t)rows;
        for (int c = 0; c < a.ncalls; ++c) {
            a.out_acc[(int64_t)c * a.cap_out + idx] = a.t.acc[(int64_t)c * a.t.entries + s];
            a.out_cnt[(int64_t)c * a.cap_out + idx] = (int64_t)(((a.rows_mask >> c) & 1u) ? rows : a.t.cnt[(int64_t)c * a.t.entries + s]);
        }
    }
}

// raw accumulators -> values: MIN / MAX un-order their images and a group without a non-NULL value is NULL; a call that only
// counts delivers its count; validity words and null counts of every call
__global__ __launch_bounds__(kBlock) void gbm_finish_kernel(const GbmFinishArgs a) {
    const int c = blockIdx.y;
    const int op = gbm_call_op(a.call_bits, c), cls = gbm_call_cls(a.call_bits, c);
    const int lane = threadIdx.x & 63;
    uint64_t* const acc = a.acc + (int64_t)c * a.cap_out;
    const int64_t* const cnt = a.cnt + (int64_t)c * a.cap_out;
    unsigned long long nulls = 0;
    const int64_t n64 = (a.n + 63) & ~(int64_t)63;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n64; i += (int64_t)gridDim.x * kBlock) {
        const bool in = i < a.n;
        bool valid = in;
        if (in) {
            const int64_t n = cnt[i];
            if (op == GBM_COUNT) acc[i] = (uint64_t)n;
            else if (op != AGG_SUM) { valid = n > 0; acc[i] = valid ? unord_bits(cls, acc[i]) : 0ull; }
        }
        const uint64_t vb = __ballot(valid), ib = __ballot(in);   // (both by the whole wave)
        if (lane == 0 && in) {
            a.validity[(int64_t)c * a.words + (i >> 6)] = vb;
            nulls += (unsigned long long)__popcll(ib & ~vb);
        }
    }
    if (lane == 0 && nulls) atomicAdd(&a.nulls[c], nulls);
}

// ------------------------------------------------------------------------------------------------
// launchers

hipError_t launch_gbm_stream(const GbmArgs& a, int rows_per_thread, int grid, size_t lds_bytes, hipStream_t s) {
    auto go = [&](auto kernel) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kGbmBlock), lds_bytes, s, a);
    };
    if (lds_bytes > (size_t)kGbmLdsBudget || a.nsubs < 1) return hipErrorInvalidValue;
    if (rows_per_thread == 4 && a.nvalues <= 2) go(gbm_stream_kernel<4, 2>);
    else if (rows_per_thread == 2 && a.nvalues <= 4) go(gbm_stream_kernel<2, 4>);
    else if (rows_per_thread == 1 && a.nvalues <= 8) go(gbm_stream_kernel<1, 8>);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
hipError_t launch_gbm_table(const GbmArgs& a, int rows_per_thread, hipStream_t s) {
    if (a.nsubs < 1) return hipErrorInvalidValue;
    int64_t grid = (a.nsubs + rows_per_thread - 1) / rows_per_thread;
    if (grid > eval_grid_limit() / 2) grid = eval_grid_limit() / 2;
    if (grid < 1) grid = 1;
    if (rows_per_thread == 4 && a.nvalues <= 2) hipLaunchKernelGGL((gbm_table_kernel<4, 2>), dim3((unsigned)grid), dim3(kGbmBlock), 0, s, a);
    else if (rows_per_thread == 2 && a.nvalues <= 4) hipLaunchKernelGGL((gbm_table_kernel<2, 4>), dim3((unsigned)grid), dim3(kGbmBlock), 0, s, a);
    else if (rows_per_thread == 1 && a.nvalues <= 8) hipLaunchKernelGGL((gbm_table_kernel<1, 8>), dim3((unsigned)grid), dim3(kGbmBlock), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
static int gbm_rows_grid(int64_t n) {
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g > eval_grid_limit()) g = eval_grid_limit();
    return g < 1 ? 1 : (int)g;
}
hipError_t launch_gbm_emit(const GbmEmitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(gbm_emit_kernel, dim3(gbm_rows_grid(a.t.entries)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_gbm_finish(const GbmFinishArgs& a, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(gbm_finish_kernel, dim3(std::min(gbm_rows_grid(a.n), 4096), a.ncalls), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rdfk
