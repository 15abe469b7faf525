// rdf_utf8.hip — Utf8 (StringArray) columns on the device: filter, take, the trims, substring, lower / upper.
//
// Every operator is one byte-gather in three steps (host side: rdf_capi_utf8.inc):
//   1. span   one lane per candidate row (an input row, or an index for take) resolves its chunk and row, and writes the
//             row's output span: the address of its first source byte, its output length, its validity, and for filter
//             whether the row is kept.  The trims look at the ends of the row only; substring walks lead bytes; lower /
//             upper walk the row once to size the mapped text and flag rows with a byte >= 0x80 ("wide" rows).
//   2. scan   of the lengths (and of the kept flags) -> every output row's byte position; the host reads the per-chunk
//             totals, applies the sizing rule, and only then is anything written to the caller's buffers.
//   3. write  offsets + validity per output row, then a copy driven by the DESTINATION: each lane owns one aligned 16-byte
//             piece of the output, finds its source row by a search over the tile's output offsets in LDS, gathers the
//             bytes (unaligned loads) and stores the piece in one full-width store.  Skewed or long strings do not
//             diverge the stores.  ASCII rows of lower / upper are mapped inside that copy, byte for byte; wide rows are
//             rewritten afterwards by a lane per row through the case tables (rdf_unicode_case.h), and only rows that
//             hold U+03A3 walk their context for the Final_Sigma rule.
#include "rdf_utf8.h"
#include "rdf_unicode_case.h"

namespace {

__device__ __forceinline__ bool bit_at(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }

// last chunk whose first row is <= row (empty chunks share the first row of the next one and are skipped by this rule)
__device__ int64_t find_chunk(const Utf8Chunk* ch, int64_t nch, int64_t row) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ch[mid].row_start <= row) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
__device__ int64_t find_out(const Utf8OutChunk* oc, int64_t n, int64_t tile) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (oc[mid].tile_start <= tile) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// ---- UTF-8: every read is bounded by the row's end (Arrow guarantees valid UTF-8; broken input must not read past the row)
__device__ __forceinline__ int lead_len(uint32_t b0) { return b0 < 0xC0 ? 1 : b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4; }
__device__ __forceinline__ uint32_t decode(const uint8_t* p, const uint8_t* e, int* n) {
    const uint32_t b0 = p[0];
    if (b0 < 0x80) { *n = 1; return b0; }
    int L = lead_len(b0);
    if (L > e - p) L = (int)(e - p);
    uint32_t cp = b0 & (b0 >= 0xF0 ? 0x07u : b0 >= 0xE0 ? 0x0Fu : 0x1Fu);
    for (int k = 1; k < L; ++k) cp = (cp << 6) | (p[k] & 0x3Fu);
    *n = L;
    return cp;
}
// start of the code point that ends at `q` (exclusive), not before b
__device__ __forceinline__ const uint8_t* prev_start(const uint8_t* b, const uint8_t* q) {
    const uint8_t* k = q - 1;
    while (k > b && (*k & 0xC0) == 0x80 && q - k < 4) --k;
    return k;
}
__device__ __forceinline__ int enc_len(uint32_t cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }
__device__ __forceinline__ uint8_t* encode(uint32_t cp, uint8_t* d, const uint8_t* dend) {
    uint8_t t[4];
    int n;
    if (cp < 0x80) { t[0] = (uint8_t)cp; n = 1; }
    else if (cp < 0x800) { t[0] = (uint8_t)(0xC0 | (cp >> 6)); t[1] = (uint8_t)(0x80 | (cp & 0x3F)); n = 2; }
    else if (cp < 0x10000) { t[0] = (uint8_t)(0xE0 | (cp >> 12)); t[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); t[2] = (uint8_t)(0x80 | (cp & 0x3F)); n = 3; }
    else { t[0] = (uint8_t)(0xF0 | (cp >> 18)); t[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F)); t[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); t[3] = (uint8_t)(0x80 | (cp & 0x3F)); n = 4; }
    for (int k = 0; k < n && d < dend; ++k) *d++ = t[k];
    return d;
}

// Unicode White_Space = Rust's char::is_whitespace
__device__ __forceinline__ bool is_ws(uint32_t c) {
    if (c <= 0x20) return c == 0x20 || (c >= 0x09 && c <= 0x0D);
    if (c < 0x85) return false;
    return c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) || c == 0x2028 || c == 0x2029 ||
           c == 0x202F || c == 0x205F || c == 0x3000;
}

// ---- case tables
__device__ __forceinline__ int64_t last_le(const uint32_t* starts, int n, uint32_t c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= c) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
// the full mapping of c: number of code points written to m (1..3)
__device__ int case_map(uint32_t c, bool upper, uint32_t m[3]) {
    const uint32_t* st = upper ? k_upper_start : k_lower_start;
    const uint32_t* info = upper ? k_upper_info : k_lower_info;
    const int32_t* delta = upper ? k_upper_delta : k_lower_delta;
    const int i = (int)last_le(st, upper ? RDF_CASE_UPPER_RUNS : RDF_CASE_LOWER_RUNS, c);
    m[0] = c;
    if (i < 0) return 1;
    const uint32_t inf = info[i], d = c - st[i];
    const uint32_t stride = (inf & RDF_CASE_FLAG_STRIDE2) ? 2u : 1u;
    if (d % stride != 0 || d / stride >= (inf & RDF_CASE_COUNT_MASK)) return 1;
    if (inf & RDF_CASE_FLAG_MULTI) {
        const uint32_t* e = (upper ? k_upper_multi : k_lower_multi) + 4 * delta[i];
        m[0] = e[1]; m[1] = e[2]; m[2] = e[3];
        return (int)e[0];
    }
    m[0] = (uint32_t)((int32_t)c + delta[i]);
    return 1;
}
__device__ __forceinline__ bool in_ranges(const uint32_t* lo, const uint32_t* hi, int n, uint32_t c) {
    const int64_t i = last_le(lo, n, c);
    return i >= 0 && c <= hi[i];
}
__device__ __forceinline__ bool is_cased(uint32_t c) { return in_ranges(k_cased_lo, k_cased_hi, RDF_CASED_RANGES, c); }
__device__ __forceinline__ bool is_case_ignorable(uint32_t c) {
    return in_ranges(k_case_ignorable_lo, k_case_ignorable_hi, RDF_CASE_IGNORABLE_RANGES, c);
}
// Final_Sigma (Unicode 3.13, Table 3-17): a cased letter before the sigma and none after it, case-ignorable ones skipped
__device__ bool final_sigma(const uint8_t* b, const uint8_t* s, const uint8_t* e) {
    const uint8_t* q = s;
    bool before = false;
    while (q > b) {
        const uint8_t* k = prev_start(b, q);
        int n;
        const uint32_t c = decode(k, q, &n);
        q = k;
        if (is_case_ignorable(c)) continue;
        before = is_cased(c);
        break;
    }
    if (!before) return false;
    int n;
    decode(s, e, &n);
    for (const uint8_t* p = s + n; p < e; p += n) {
        const uint32_t c = decode(p, e, &n);
        if (is_case_ignorable(c)) continue;
        return !is_cased(c);
    }
    return true;
}
// mapped bytes of one code point (the sigma's two forms are both two bytes)
__device__ __forceinline__ int mapped_len(uint32_t c, bool upper) {
    uint32_t m[3];
    const int k = case_map(c, upper, m);
    int L = 0;
    for (int j = 0; j < k; ++j) L += enc_len(m[j]);
    return L;
}

__device__ __forceinline__ int64_t grid_stride_start() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t grid_stride() { return (int64_t)gridDim.x * blockDim.x; }

// ---- 1. span
__global__ void utf8_bounds_kernel(Utf8Args a) {
    for (int64_t c = grid_stride_start(); c < a.nchunks; c += grid_stride()) {
        a.bounds[2 * c] = a.chunks[c].offs[0];
        a.bounds[2 * c + 1] = a.chunks[c].offs[a.chunks[c].rows];
    }
}

__global__ void utf8_span_kernel(Utf8Args a) {
    for (int64_t g = grid_stride_start(); g < a.n; g += grid_stride()) {
        int64_t row = g;
        bool keep = true, ok = true;
        if (a.op == UTF8_TAKE) {
            const int64_t ii = a.idx_off + g;
            ok = !a.idx_valid || bit_at(a.idx_valid, ii);
            row = ok ? (a.idx64 ? (int64_t)((const uint64_t*)a.idx)[ii] : (int64_t)((const uint32_t*)a.idx)[ii]) : 0;
            if (ok && (row < 0 || row >= a.total_rows)) {   // (u64 indices beyond 2^63 read as negative)
                atomicOr(a.err, 1u);
                ok = false;
            }
        }
        const uint8_t *b = nullptr, *e = nullptr;
        if (ok) {
            const Utf8Chunk& c = a.chunks[find_chunk(a.chunks, a.nchunks, row)];
            const int64_t r = row - c.row_start;
            if (a.op == UTF8_FILTER) keep = bit_at(c.mask, c.mask_off + r) && (!c.mask_valid || bit_at(c.mask_valid, c.mask_off + r));
            ok = !c.valid || bit_at(c.valid, c.valid_off + r);
            int32_t o0 = c.offs[r], o1 = c.offs[r + 1];
            o0 = min(max(o0, c.lo), c.hi);
            o1 = min(max(o1, o0), c.hi);
            b = c.data + o0;
            e = c.data + o1;
        }
        uint8_t fl = 0;
        int64_t len = 0;
        if (ok && keep) {
            fl = UTF8_ROW_VALID;
            switch (a.op) {
            case UTF8_TRIM: case UTF8_LTRIM: case UTF8_RTRIM: {
                if (a.op != UTF8_RTRIM)
                    while (b < e) {
                        int n;
                        const uint32_t c = decode(b, e, &n);
                        if (!is_ws(c)) break;
                        b += n;
                    }
                if (a.op != UTF8_LTRIM)
                    while (e > b) {
                        const uint8_t* k = prev_start(b, e);
                        int n;
                        if (!is_ws(decode(k, e, &n))) break;
                        e = k;
                    }
                break;
            }
            case UTF8_SUBSTRING: {   // chars().skip(pos).take(len): code points are counted by their lead bytes
                const uint8_t* p = b;
                for (int32_t i = 0; i < a.pos && p < e; ++i) p += min((int64_t)lead_len(*p), (int64_t)(e - p));
                const uint8_t* q = p;
                for (int32_t i = 0; i < a.len && q < e; ++i) q += min((int64_t)lead_len(*q), (int64_t)(e - q));
                b = p; e = q;
                break;
            }
            case UTF8_LOWER: case UTF8_UPPER: {
                const bool up = a.op == UTF8_UPPER;
                int64_t L = 0;
                for (const uint8_t* p = b; p < e;) {
                    if (*p < 0x80) { ++L; ++p; continue; }
                    fl |= UTF8_ROW_WIDE;
                    int n;
                    L += mapped_len(decode(p, e, &n), up);
                    p += n;
                }
                len = L;
                break;
            }
            default: break;
            }
            if (a.op != UTF8_LOWER && a.op != UTF8_UPPER) len = e - b;
        }
        if (a.op == UTF8_FILTER) a.keep[g] = keep ? 1 : 0;
        a.blen[g] = len;
        a.src[g] = (uint64_t)(uintptr_t)b;
        a.flags[g] = fl;
    }
}

// ---- 2. per output chunk totals (after the scans)
__global__ void utf8_totals_kernel(Utf8Args a) {
    for (int64_t c = grid_stride_start(); c < a.nout; c += grid_stride()) {
        if (a.op == UTF8_TAKE) { a.tot[0] = a.bscan[a.n]; a.tot[1] = a.n; continue; }
        const int64_t s = a.chunks[c].row_start, e = s + a.chunks[c].rows;
        a.tot[2 * c] = a.bscan[e] - a.bscan[s];
        a.tot[2 * c + 1] = a.op == UTF8_FILTER ? a.rscan[e] - a.rscan[s] : a.chunks[c].rows;
    }
}

// ---- 3. write
// validity cleared, the closing offset of every output chunk (also of empty ones)
__global__ void utf8_prep_kernel(Utf8Args a) {
    for (int64_t c = blockIdx.x; c < a.nout; c += gridDim.x) {
        const Utf8OutChunk& o = a.outs[c];
        if (threadIdx.x == 0) o.offs[o.rows] = (int32_t)o.bytes;
        if (o.valid)
            for (int64_t k = threadIdx.x; k < (o.rows + 7) / 8; k += blockDim.x) o.valid[k] = 0;
    }
}

__global__ void utf8_place_kernel(Utf8Args a) {
    for (int64_t g = grid_stride_start(); g < a.n; g += grid_stride()) {
        int64_t oc = 0, orow = g;
        if (a.op != UTF8_TAKE) {
            oc = find_chunk(a.chunks, a.nchunks, g);
            if (a.op == UTF8_FILTER) {
                if (!a.keep[g]) continue;
                orow = a.rscan[g];
            }
        }
        const Utf8OutChunk& o = a.outs[oc];
        const int64_t r = orow - o.row_start;
        o.offs[r] = (int32_t)(a.bscan[g] - o.byte_start);
        const uint8_t fl = a.flags[g];
        if (fl & UTF8_ROW_VALID) {
            if (o.valid) atomicOr((unsigned int*)(o.valid + ((r >> 3) & ~(int64_t)3)), 1u << (r & 31));
        } else atomicAdd(a.null_counts + oc, 1ull);
        a.osrc[orow] = a.src[g];
        a.oflags[orow] = fl;
        // the copy tiles that start inside this row learn their first row here, so no copy block has to search for it
        const int64_t b0 = a.bscan[g] - o.byte_start, b1 = b0 + a.blen[g];
        for (int64_t t = (b0 + kUtf8CopyTile - 1) / kUtf8CopyTile; t * kUtf8CopyTile < b1; ++t) a.tile_row[o.tile_start + t] = r;
    }
}

__device__ __forceinline__ uint8_t ascii_case(uint8_t c, int op) {
    if (op == UTF8_LOWER) return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c;
    if (op == UTF8_UPPER) return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
    return c;
}

// one block per kUtf8CopyTile output bytes of one output chunk; lane t owns bytes [lo + 16 t, lo + 16 t + 16)
__global__ void __launch_bounds__(kUtf8CopyThreads) utf8_copy_kernel(Utf8Args a) {
    __shared__ int32_t s_off[kUtf8WindowRows + 1];
    __shared__ uint64_t s_src[kUtf8WindowRows];
    __shared__ uint8_t s_fl[kUtf8WindowRows];
    __shared__ uint4 s_buf[kUtf8CopyThreads];
    __shared__ int64_t s_meta[5];
    const int64_t tile = blockIdx.x;
    const int t = threadIdx.x;
    if (t == 0) {
        const int64_t oc = find_out(a.outs, a.nout, tile);
        const Utf8OutChunk& o = a.outs[oc];
        const int64_t lt = tile - o.tile_start, lo = lt * kUtf8CopyTile, hi = min(lo + (int64_t)kUtf8CopyTile, o.bytes);
        // rows lo .. the row of the next tile's first byte (the chunk's last row for its last tile) hold the tile's bytes
        const int64_t r0 = a.tile_row[tile];
        const int64_t r1 = hi < o.bytes ? a.tile_row[tile + 1] : o.rows - 1;
        s_meta[0] = oc; s_meta[1] = lo; s_meta[2] = hi; s_meta[3] = r0; s_meta[4] = r1 - r0 + 1;
    }
    __syncthreads();
    const Utf8OutChunk& o = a.outs[s_meta[0]];
    const int64_t lo = s_meta[1], hi = s_meta[2];
    const int64_t r0 = s_meta[3], nwin = s_meta[4];
    const bool inwin = nwin <= kUtf8WindowRows;
    if (inwin) {
        for (int64_t k = t; k <= nwin; k += kUtf8CopyThreads) s_off[k] = o.offs[r0 + k];
        for (int64_t k = t; k < nwin; k += kUtf8CopyThreads) {
            s_src[k] = a.osrc[o.row_start + r0 + k];
            s_fl[k] = a.oflags[o.row_start + r0 + k];
        }
    }
    __syncthreads();
    const int64_t p0 = lo + 16 * (int64_t)t;
    if (p0 >= hi) return;
    const int64_t pend = min(p0 + 16, hi);
    uint8_t* mine = (uint8_t*)&s_buf[t];
    auto off_at = [&](int64_t k) -> int64_t { return inwin ? s_off[k] : o.offs[r0 + k]; };
    // window row holding p0
    int64_t l = 0, h = nwin + 1;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (off_at(mid) <= p0) l = mid + 1; else h = mid;
    }
    int64_t k = l - 1;
    int64_t p = p0;
    while (p < pend) {
        int64_t next = off_at(k + 1);
        while (next <= p) { ++k; next = off_at(k + 1); }
        const int64_t rb = off_at(k), re = min(next, pend);
        const uint64_t sa = inwin ? s_src[k] : a.osrc[o.row_start + r0 + k];
        const uint8_t fl = inwin ? s_fl[k] : a.oflags[o.row_start + r0 + k];
        const uint8_t* src = (const uint8_t*)(uintptr_t)sa + (p - rb);
        if (fl & UTF8_ROW_WIDE) {   // rewritten by utf8_wide_kernel
            for (; p < re; ++p) mine[p - p0] = 0;
        } else {
            for (; p < re; ++p, ++src) mine[p - p0] = ascii_case(*src, a.op);
        }
    }
    uint8_t* dst = o.data + p0;
    if (pend - p0 == 16 && ((uintptr_t)dst & 15) == 0) *(uint4*)dst = s_buf[t];
    else for (int64_t q = 0; q < pend - p0; ++q) dst[q] = mine[q];
}

// lower / upper of the rows with a byte >= 0x80, a lane per row
__global__ void utf8_wide_kernel(Utf8Args a) {
    const bool up = a.op == UTF8_UPPER;
    for (int64_t g = grid_stride_start(); g < a.n; g += grid_stride()) {
        if (!(a.flags[g] & UTF8_ROW_WIDE)) continue;
        const int64_t ci = find_chunk(a.chunks, a.nchunks, g);
        const Utf8Chunk& c = a.chunks[ci];
        const Utf8OutChunk& o = a.outs[ci];
        const int64_t r = g - c.row_start;
        int32_t o0 = c.offs[r], o1 = c.offs[r + 1];
        o0 = min(max(o0, c.lo), c.hi);
        o1 = min(max(o1, o0), c.hi);
        const uint8_t *b = c.data + o0, *e = c.data + o1;
        uint8_t* d = o.data + (a.bscan[g] - o.byte_start);
        const uint8_t* dend = d + a.blen[g];
        for (const uint8_t* p = b; p < e;) {
            int n;
            const uint32_t cp = decode(p, e, &n);
            if (cp == 0x3A3 && !up) d = encode(final_sigma(b, p, e) ? 0x3C2 : 0x3C3, d, dend);
            else {
                uint32_t m[3];
                const int km = case_map(cp, up, m);
                for (int j = 0; j < km; ++j) d = encode(m[j], d, dend);
            }
            p += n;
        }
    }
}

unsigned grid_for(int64_t n, int threads) {
    const int64_t b = (n + threads - 1) / threads;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

}  // namespace

hipError_t launch_utf8_bounds(const Utf8Args& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_bounds_kernel, dim3(grid_for(a.nchunks, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_span(const Utf8Args& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_span_kernel, dim3(grid_for(a.n, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_totals(const Utf8Args& a, hipStream_t s) {
    if (a.nout <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_totals_kernel, dim3(grid_for(a.nout, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_write(const Utf8Args& a, hipStream_t s) {
    if (a.nout <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_prep_kernel, dim3((unsigned)(a.nout < 65536 ? a.nout : 65536)), dim3(256), 0, s, a);
    if (a.n > 0) hipLaunchKernelGGL(utf8_place_kernel, dim3(grid_for(a.n, 256)), dim3(256), 0, s, a);
    if (a.ntiles > 0) hipLaunchKernelGGL(utf8_copy_kernel, dim3((unsigned)a.ntiles), dim3(kUtf8CopyThreads), 0, s, a);
    if (a.n > 0 && (a.op == UTF8_LOWER || a.op == UTF8_UPPER))
        hipLaunchKernelGGL(utf8_wide_kernel, dim3(grid_for(a.n, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
