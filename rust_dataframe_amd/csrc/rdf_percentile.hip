// rdf_percentile.hip — the pick of rdf_groupby_percentile (host side: rdf_capi_percentile.inc, the decisions about one group
// and one call: rdf_percentile.h, argument block: rdf_device.h).
//
// The window front has ordered the rows by (grouping keys, value): group g is the partition pstart[g] .. pstart[g + 1], its
// values ascend inside it, and NULL values sort last, so the group's NULL run is its last peer group or absent.  With
// (scan[j + 1] & 0xFFFFFFFF) - 1 the peer group of sorted position j and gstart[h] the head of peer group h, everything one
// (group, call) needs is a handful of loads:
//   m       the extent of the group, minus the last peer group when the row at its head is NULL
//   CONT    the values at positions lo and hi of the group, gathered through perm and the staged chunk tables; the two are
//           peers exactly when they lie in one peer group
//   DISC    the head of the peer group of position k: ties keep ascending row order, so perm[head] is the smallest row index
//           among the peers of the k-th value
// One thread per (group, call): O(1) each, wherever the group boundaries fall, and no row is read that is not an answer.
// Nothing is accumulated, so equal inputs give equal bytes; the one atomic is an integer count of NULL results.
#include "rdf_percentile.h"
#include "rdf_utf8.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

// The value of `row` as its own bits, zero-extended; *isnull: the row is NULL (nothing else is read then).
__device__ __forceinline__ uint64_t pct_value(const PctPickArgs& a, double inv, int64_t row, bool* isnull) {
    int64_t c = 0, start = 0;
    if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
    if (a.vutf8) {
        const Utf8Chunk& u = a.vutf8[c];
        const int64_t e = u.valid_off + row - start;
        *isnull = u.valid ? !((u.valid[e >> 3] >> (e & 7)) & 1) : false;
        return 0;
    }
    const DevChunkCol cc = a.vchunks[c];
    const int64_t e = cc.offset + row - start;
    *isnull = cc.validity ? !((cc.validity[e >> 3] >> (e & 7)) & 1) : false;
    if (*isnull) return 0;
    switch (a.vdtype) {
        case RDF_I8: case RDF_U8: return as_global<uint8_t>(cc.values)[e];
        case RDF_I16: case RDF_U16: return as_global<uint16_t>(cc.values)[e];
        case RDF_I32: case RDF_U32: case RDF_F32: return as_global<uint32_t>(cc.values)[e];
        default: return as_global<uint64_t>(cc.values)[e];
    }
}

__device__ __forceinline__ int64_t pct_peer(const PctPickArgs& a, int64_t j) { return (int64_t)(uint32_t)(uint64_t)a.scan[j + 1] - 1; }
__device__ __forceinline__ int64_t pct_row(const PctPickArgs& a, int64_t j) { return a.perm ? (int64_t)a.perm[j] : j; }

__global__ __launch_bounds__(kPctThreads) void pct_pick_kernel(const PctPickArgs a) {
    const int ncalls = a.ncalls > 0 ? a.ncalls : 1;      // no calls: one thread per group writes the count
    const int64_t t = (int64_t)blockIdx.x * kPctThreads + threadIdx.x;
    if (t >= a.groups * ncalls) return;
    const int64_t g = t / ncalls;
    const int c = (int)(t - g * ncalls);
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t s0 = a.pstart[g], s1 = a.pstart[g + 1];
    int64_t m = s1 - s0;
    if (a.nullable) {
        const int64_t head = a.gstart[pct_peer(a, s1 - 1)];
        bool isnull = false;
        pct_value(a, inv, pct_row(a, head), &isnull);
        if (isnull) m = head - s0;
    }
    if (c == 0 && a.counts) a.counts[g] = m;
    if (a.ncalls <= 0) return;
    const PctCallOut& o = a.calls[c];
    if (o.vbytes) o.vbytes[g] = m > 0 ? 1 : 0;
    if (m <= 0) {
        if (o.kind == PCT_CONT) as_global_mut<uint64_t>(o.values)[g] = 0;
        else as_global_mut<uint32_t>(o.values)[g] = 0;
        atomicAdd(&a.nulls[c], 1ull);
        return;
    }
    if (o.kind == PCT_CONT) {
        const PctRank r = pct_rank(m, o.p);
        bool isnull = false;
        const double dlo = pct_d(a.vdtype, pct_value(a, inv, pct_row(a, s0 + r.lo), &isnull));
        double dhi = dlo;
        bool peers = true;
        if (r.hi != r.lo) {
            peers = pct_peer(a, s0 + r.lo) == pct_peer(a, s0 + r.hi);
            if (!peers) dhi = pct_d(a.vdtype, pct_value(a, inv, pct_row(a, s0 + r.hi), &isnull));
        }
        as_global_mut<uint64_t>(o.values)[g] = pct_interpolate(r, dlo, dhi, peers);
    } else {
        const int64_t k = pct_disc_index(m, o.p);
        as_global_mut<uint32_t>(o.values)[g] = (uint32_t)pct_row(a, a.gstart[pct_peer(a, s0 + k)]);
    }
}

// ================================================================ the select route: one whole numeric column, no sort
// Keys are the ordered unsigned images of the values at the dtype's own width (pct_key).  Up to 16 target ranks are narrowed
// one digit of kPctSelBits per pass, most significant first:
//   hist     one streaming read of values and validity.  A row is a candidate when the digits decided so far equal the prefix
//            of some slot; the block counts candidates per (slot, next digit) in LDS and merges into the state with integer
//            atomics.  Lanes of a wave that hit the same counter are combined first (two leader-and-ballot turns): an
//            all-equal or two-valued column costs one or two LDS atomics per wave and row, not 64 serialized ones.
//   plan     one block: every rank's bucket and residual by pct_plan_bucket, the distinct (slot, bucket) pairs become the new
//            slots.  Pass 0 also takes m and the ranks themselves (pct_rank / pct_disc_index), so nothing returns to the
//            host.  When the digits are used up the prefix IS the key; when all slots together hold at most kPctSelFinish
//            candidates the phase becomes FINISH.  Every later hist launch finds the phase changed and returns at once.
//   gather   phase FINISH: one more read collects the candidates' keys; finish: one block sorts them in LDS (bitonic) — whole
//            keys, so every slot is one run of the sorted list — and reads every rank at (start of its slot) + residual.
//   rows     DISC only: the smallest row index holding the resolved key, an integer atomicMin after a wave-level minimum.
//   emit     d(), the interpolation, validity bytes, the count.
// Candidates are re-read under the prefix test, not compacted: the passes are bounded by ceil(key bits / digit bits) hist
// reads plus one gather whatever the values hold, need no memory that depends on the data, and a bucket holding every row
// (an all-equal column) costs what any other pass costs.  Only integer atomics; no value goes through one, so the result is a
// function of the multiset of rows.

struct PctSelRow { uint64_t key; bool live; };

// Row `row` of the column: its key, and whether it is a non-NULL row inside the column.  No branch depends on a loaded
// value (a row beyond the column reads the last row, a NULL row's value is read and dropped), so the loads of a whole tile
// can be in flight together.
__device__ __forceinline__ PctSelRow pct_sel_row(const PctSelArgs& a, double inv, int64_t row) {
    const bool inside = row < a.n;
    if (!inside) row = a.n - 1;
    int64_t c = 0, start = 0;
    if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
    const DevChunkCol cc = a.vchunks[c];
    const int64_t e = cc.offset + row - start;
    const uint32_t vb = cc.validity ? (uint32_t)cc.validity[e >> 3] : 0xFFu;
    uint64_t raw;
    switch (a.key_bits) {
        case 8: raw = as_global<uint8_t>(cc.values)[e]; break;
        case 16: raw = as_global<uint16_t>(cc.values)[e]; break;
        case 32: raw = as_global<uint32_t>(cc.values)[e]; break;
        default: raw = as_global<uint64_t>(cc.values)[e]; break;
    }
    PctSelRow r;
    r.key = pct_key(a.vdtype, raw);
    r.live = inside && ((vb >> (e & 7)) & 1u);
    return r;
}

// This thread's rows of the tile at `base` come in batches of kPctSelBatch: entry k of batch b is row
// base + (b * kPctSelBatch + k) * kPctSelThreads + tid.  -> their keys, and as the result one bit per live row.  A batch's
// loads are in flight together; four of them keep the kernels at 8 waves a SIMD, which the dependent scalar / vector steps
// of the counting need more than they need longer batches (measured: batches of 16 at 3 waves a SIMD ran 1.7 x slower).
constexpr int kPctSelPer = kPctSelTile / kPctSelThreads;
constexpr int kPctSelBatch = 4;
static_assert(kPctSelPer * kPctSelThreads == kPctSelTile && kPctSelPer % kPctSelBatch == 0, "whole blocks per tile, whole batches per thread");
__device__ __forceinline__ uint32_t pct_sel_batch(const PctSelArgs& a, double inv, int64_t base, int batch, int tid, uint64_t (&key)[kPctSelBatch]) {
    uint32_t live = 0;
#pragma unroll
    for (int k = 0; k < kPctSelBatch; ++k) {
        const PctSelRow r = pct_sel_row(a, inv, base + (int64_t)(batch * kPctSelBatch + k) * kPctSelThreads + tid);
        key[k] = r.key;
        live |= (uint32_t)r.live << k;
    }
    return live;
}

// The slot whose prefix the key's first `done` digits equal, or -1.  (done == 0: the one slot of the empty prefix.)
__device__ __forceinline__ int pct_sel_slot(const uint64_t* prefix, int nslots, uint64_t key, int key_bits, int done) {
    if (done == 0) return 0;
    const uint64_t pre = key >> (key_bits - done * kPctSelBits);
    int s = -1;
    for (int j = 0; j < nslots; ++j)
        if (prefix[j] == pre) s = j;
    return s;
}

__global__ __launch_bounds__(kPctSelThreads) void pct_sel_hist_kernel(const PctSelArgs a) {
    __shared__ uint32_t lh[kPctSelRanks * kPctSelBuckets];
    __shared__ uint64_t spre[kPctSelRanks];
    PctSelState* st = a.st;
    if (st->phase != PCT_SEL_NARROW || st->digits_done != a.pass) return;     // (uniform: written by the plan launch before this one)
    const int tid = threadIdx.x, lane = tid & 63;
    const int nslots = a.pass == 0 ? 1 : st->nslots;
    for (int i = tid; i < nslots * kPctSelBuckets; i += kPctSelThreads) lh[i] = 0;
    if (tid < kPctSelRanks) spre[tid] = st->prefix[tid];
    __syncthreads();
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int shift = a.key_bits - (a.pass + 1) * kPctSelBits;
    const int64_t ntiles = (a.n + kPctSelTile - 1) / kPctSelTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
        for (int batch = 0; batch < kPctSelPer / kPctSelBatch; ++batch) {
            uint64_t key[kPctSelBatch];
            const uint32_t live = pct_sel_batch(a, inv, tile * kPctSelTile, batch, tid, key);
#pragma unroll
            for (int k = 0; k < kPctSelBatch; ++k) {
                const int slot = (live >> k) & 1u ? pct_sel_slot(spre, nslots, key[k], a.key_bits, a.pass) : -1;
                const bool active = slot >= 0;
                const uint32_t bin = active ? (uint32_t)slot * kPctSelBuckets + (uint32_t)((key[k] >> shift) & (kPctSelBuckets - 1)) : 0u;
                // lanes that hit one counter are combined first: twice the lowest lane still waiting names its counter, the
                // lanes with the same one are counted by a ballot and leave.  An all-equal column is done after the first
                // turn, a two-valued one after the second; what is left (a column of many values) adds lane by lane to
                // counters that mostly differ.
                uint64_t waiting = __ballot(active);
#pragma unroll
                for (int turn = 0; turn < 2; ++turn) {
                    if (!waiting) break;                               // (wave-uniform)
                    const int leader = __ffsll((long long)waiting) - 1;
                    const uint32_t lbin = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
                    const uint64_t same = __ballot(active && bin == lbin) & waiting;
                    if (lane == leader) atomicAdd(&lh[lbin], (uint32_t)__popcll(same));
                    waiting &= ~same;
                }
                if ((waiting >> lane) & 1ull) atomicAdd(&lh[bin], 1u);
            }
        }
    __syncthreads();
    for (int i = tid; i < nslots * kPctSelBuckets; i += kPctSelThreads)
        if (lh[i]) atomicAdd(&st->hist[0][0] + i, lh[i]);
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&st->passes, 1);
}

__global__ __launch_bounds__(kPctSelThreads) void pct_sel_plan_kernel(const PctSelArgs a) {
    __shared__ uint64_t npre[kPctSelRanks], ncnt[kPctSelRanks];
    PctSelState* st = a.st;
    const int tid = threadIdx.x;
    if (st->phase != PCT_SEL_NARROW || st->digits_done != a.pass) return;
    const int nranks = 2 * a.ncalls;
    if (a.pass == 0) {
        __shared__ uint64_t sm;
        if (tid == 0) {
            uint64_t m = 0;
            for (int b = 0; b < kPctSelBuckets; ++b) m += st->hist[0][b];
            st->m = m;
            sm = m;
            if (m == 0) st->phase = PCT_SEL_RESOLVED;
        }
        __syncthreads();
        const uint64_t m = sm;
        if (m == 0) return;
        if (tid < a.ncalls) {
            const PctCallOut& o = a.calls[tid];
            int64_t lo, hi;
            if (o.kind == PCT_CONT) { const PctRank r = pct_rank((int64_t)m, o.p); lo = r.lo; hi = r.hi; }
            else lo = hi = pct_disc_index((int64_t)m, o.p);
            st->residual[2 * tid] = (uint64_t)lo;
            st->residual[2 * tid + 1] = (uint64_t)hi;
            st->slot[2 * tid] = st->slot[2 * tid + 1] = 0;
            st->disc_row[tid] = 0xFFFFFFFFu;
        }
        __syncthreads();
    }
    if (tid < nranks) {
        const int s = st->slot[tid];
        uint64_t res = st->residual[tid];
        const int b = pct_plan_bucket(st->hist[s], kPctSelBuckets, &res);
        npre[tid] = (a.pass == 0 ? 0ull : st->prefix[s] << kPctSelBits) | (uint64_t)b;
        ncnt[tid] = st->hist[s][b];
        st->residual[tid] = res;
    }
    __syncthreads();
    if (tid == 0) {
        int nslots = 0;
        uint64_t total = 0;
        for (int r = 0; r < nranks; ++r) {
            int j = 0;
            while (j < nslots && st->prefix[j] != npre[r]) ++j;      // (slots 0 .. nslots - 1 are already this pass's)
            if (j == nslots) { st->prefix[j] = npre[r]; total += ncnt[r]; ++nslots; }
            st->slot[r] = j;
        }
        st->nslots = nslots;
        st->digits_done = a.pass + 1;
        if ((a.pass + 1) * kPctSelBits >= a.key_bits) {               // the bits are used up: the prefix IS the key
            for (int r = 0; r < nranks; ++r) st->key[r] = st->prefix[st->slot[r]];
            st->phase = PCT_SEL_RESOLVED;
        } else if (total <= (uint64_t)kPctSelFinish) st->phase = PCT_SEL_FINISH;
    }
    __syncthreads();
    for (int i = tid; i < kPctSelRanks * kPctSelBuckets; i += kPctSelThreads) (&st->hist[0][0])[i] = 0;
}

__global__ __launch_bounds__(kPctSelThreads) void pct_sel_gather_kernel(const PctSelArgs a) {
    __shared__ uint64_t spre[kPctSelRanks];
    PctSelState* st = a.st;
    if (st->phase != PCT_SEL_FINISH) return;
    const int tid = threadIdx.x;
    const int nslots = st->nslots, done = st->digits_done;
    if (tid < kPctSelRanks) spre[tid] = st->prefix[tid];
    __syncthreads();
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t ntiles = (a.n + kPctSelTile - 1) / kPctSelTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
        for (int batch = 0; batch < kPctSelPer / kPctSelBatch; ++batch) {
            uint64_t key[kPctSelBatch];
            const uint32_t live = pct_sel_batch(a, inv, tile * kPctSelTile, batch, tid, key);
#pragma unroll
            for (int k = 0; k < kPctSelBatch; ++k) {
                if (!((live >> k) & 1u) || pct_sel_slot(spre, nslots, key[k], a.key_bits, done) < 0) continue;
                const uint32_t at = atomicAdd(&st->cand_count, 1u);       // (at most kPctSelFinish of them: the plan counted)
                if (at < (uint32_t)kPctSelFinish) st->cand[at] = key[k];
            }
        }
}

__global__ __launch_bounds__(kPctSelThreads) void pct_sel_finish_kernel(const PctSelArgs a) {
    __shared__ uint64_t keys[kPctSelFinish];
    PctSelState* st = a.st;
    if (st->phase != PCT_SEL_FINISH) return;
    const int tid = threadIdx.x;
    const uint32_t cnt = st->cand_count < (uint32_t)kPctSelFinish ? st->cand_count : (uint32_t)kPctSelFinish;
    for (int i = tid; i < kPctSelFinish; i += kPctSelThreads) keys[i] = (uint32_t)i < cnt ? st->cand[i] : ~0ull;   // the padding sorts last
    __syncthreads();
    for (int k = 2; k <= kPctSelFinish; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < kPctSelFinish; i += kPctSelThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t u = keys[i], v = keys[x];
                    if ((u > v) == ((i & k) == 0)) { keys[i] = v; keys[x] = u; }
                }
            }
            __syncthreads();
        }
    const int nranks = 2 * a.ncalls;
    if (tid < nranks && cnt > 0) {
        const int rem = a.key_bits - st->digits_done * kPctSelBits;   // 1 .. key_bits - kPctSelBits: a finish follows at least one digit
        const uint64_t first = st->prefix[st->slot[tid]] << rem;      // the smallest key of the slot
        uint32_t lo = 0, hi = cnt;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (keys[mid] < first) lo = mid + 1; else hi = mid; }
        uint64_t at = (uint64_t)lo + st->residual[tid];
        if (at > cnt - 1) at = cnt - 1;
        st->key[tid] = keys[at];
    }
    __syncthreads();
    if (tid == 0) { st->phase = PCT_SEL_RESOLVED; st->finished = 1; }
}

// A wave meets its rows in ascending order (tiles ascend, entries ascend, lanes ascend), so the first hit of a call IS the
// wave's smallest row for it, and a wave whose calls all have their hit is done: over an all-equal column every wave stops
// after its first tile.  One LDS minimum per wave and call, one global atomicMin per block and call.
__global__ __launch_bounds__(kPctSelThreads) void pct_sel_rows_kernel(const PctSelArgs a) {
    __shared__ uint32_t sbest[RDF_PERCENTILE_MAX_CALLS];
    PctSelState* st = a.st;
    if (st->phase != PCT_SEL_RESOLVED || st->m == 0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < RDF_PERCENTILE_MAX_CALLS) sbest[tid] = 0xFFFFFFFFu;
    __syncthreads();
    uint64_t want[RDF_PERCENTILE_MAX_CALLS];
    uint32_t best[RDF_PERCENTILE_MAX_CALLS];
    uint32_t pending = 0;                                              // (wave-uniform) the DISC calls without a hit yet
#pragma unroll
    for (int c = 0; c < RDF_PERCENTILE_MAX_CALLS; ++c) {
        want[c] = c < a.ncalls ? st->key[2 * c] : 0;
        best[c] = 0xFFFFFFFFu;
        if (c < a.ncalls && a.calls[c].kind == PCT_DISC) pending |= 1u << c;
    }
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t ntiles = (a.n + kPctSelTile - 1) / kPctSelTile;
    for (int64_t tile = blockIdx.x; tile < ntiles && pending; tile += gridDim.x)
        for (int batch = 0; batch < kPctSelPer / kPctSelBatch && pending; ++batch) {
            uint64_t key[kPctSelBatch];
            const uint32_t live = pct_sel_batch(a, inv, tile * kPctSelTile, batch, tid, key);
#pragma unroll
            for (int k = 0; k < kPctSelBatch; ++k) {
#pragma unroll
                for (int c = 0; c < RDF_PERCENTILE_MAX_CALLS; ++c) {
                    if (!((pending >> c) & 1u)) continue;              // (uniform)
                    const uint64_t hit = __ballot(((live >> k) & 1u) && key[k] == want[c]);
                    if (hit) {
                        best[c] = (uint32_t)(tile * kPctSelTile + (int64_t)(batch * kPctSelBatch + k) * kPctSelThreads + (tid - lane) + (__ffsll((long long)hit) - 1));
                        pending &= ~(1u << c);
                    }
                }
            }
        }
#pragma unroll
    for (int c = 0; c < RDF_PERCENTILE_MAX_CALLS; ++c)
        if (lane == 0 && best[c] != 0xFFFFFFFFu) atomicMin(&sbest[c], best[c]);
    __syncthreads();
    if (tid < RDF_PERCENTILE_MAX_CALLS && sbest[tid] != 0xFFFFFFFFu) atomicMin(&st->disc_row[tid], sbest[tid]);
}

__global__ void pct_sel_emit_kernel(const PctSelArgs a) {
    PctSelState* st = a.st;
    const int c = threadIdx.x;
    const int64_t m = (int64_t)st->m;
    if (c == 0) {
        if (a.counts) a.counts[0] = m;
        if (a.group_rows) a.group_rows[0] = 0;
    }
    if (c >= a.ncalls) return;
    const PctCallOut& o = a.calls[c];
    if (o.vbytes) o.vbytes[0] = m > 0 ? 1 : 0;
    if (m <= 0) {
        if (o.kind == PCT_CONT) as_global_mut<uint64_t>(o.values)[0] = 0;
        else as_global_mut<uint32_t>(o.values)[0] = 0;
        a.nulls[c] = 1;
        return;
    }
    if (o.kind == PCT_CONT) {
        const PctRank r = pct_rank(m, o.p);
        const uint64_t klo = st->key[2 * c], khi = st->key[2 * c + 1];
        as_global_mut<uint64_t>(o.values)[0] = pct_interpolate(r, pct_d(a.vdtype, pct_unkey(a.vdtype, klo)), pct_d(a.vdtype, pct_unkey(a.vdtype, khi)), klo == khi);
    } else {
        as_global_mut<uint32_t>(o.values)[0] = st->disc_row[c];
    }
}

}  // namespace

namespace {
int pct_sel_grid(const PctSelArgs& a) {
    const int64_t want = (a.n + kPctSelTile - 1) / kPctSelTile, lim = (int64_t)eval_grid_limit();
    return (int)(want > lim ? lim : (want < 1 ? 1 : want));
}
}  // namespace

hipError_t launch_pct_sel_hist(const PctSelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pct_sel_hist_kernel, dim3((unsigned)pct_sel_grid(a)), dim3(kPctSelThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_pct_sel_plan(const PctSelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pct_sel_plan_kernel, dim3(1), dim3(kPctSelThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_pct_sel_gather(const PctSelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pct_sel_gather_kernel, dim3((unsigned)pct_sel_grid(a)), dim3(kPctSelThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_pct_sel_finish(const PctSelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pct_sel_finish_kernel, dim3(1), dim3(kPctSelThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_pct_sel_rows(const PctSelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pct_sel_rows_kernel, dim3((unsigned)pct_sel_grid(a)), dim3(kPctSelThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_pct_sel_emit(const PctSelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pct_sel_emit_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pct_pick(const PctPickArgs& a, hipStream_t s) {
    const int64_t threads = a.groups * (a.ncalls > 0 ? a.ncalls : 1);
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(pct_pick_kernel, dim3((unsigned)((threads + kPctThreads - 1) / kPctThreads)), dim3(kPctThreads), 0, s, a);
    return hipGetLastError();
}
