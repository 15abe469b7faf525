// ubench_hist16.hip — should a 16-bit column be answered from ONE histogram?  The select route of
// rdf_groupby_percentile counts 8 bits a pass in LDS, so a 16-bit key takes two reads; 65 536 32-bit counters do not fit LDS,
// so the one-read form has to count in global memory.  Two kernels over the same n UInt16 keys, both with the library's
// two-turn combine of lanes that hit one counter:
//   lds8x2    two passes: the top digit into 256 LDS counters merged per block, then the low digit of the rows whose top digit is
//             the median's (the shape of pct_sel_hist_kernel's passes 0 and 1, without validity and slots)
//   global16  one pass: every row adds to one of 65 536 counters in global memory
// over three columns: uniform keys, all keys equal, two values.  Both are checked against each other (the median key).
//
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/ubench_hist16.bin tools/ubench_hist16.hip
// Run:   tools/ubench_hist16.bin [rows=5e7] [reps=5]       (one JSON line per column and variant, best of reps)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                                   \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                            \
        }                                                                                       \
    } while (0)

constexpr int kThreads = 256, kTile = 4096, kPer = kTile / kThreads, kBatch = 4;

__global__ void fill_kernel(uint16_t* keys, int64_t n, int kind) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t h = (uint64_t)i * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        keys[i] = kind == 0 ? (uint16_t)h : kind == 1 ? (uint16_t)42 : ((h & 3) ? (uint16_t)65529 : (uint16_t)7);
    }
}

// counters[bin] += 1 for every active lane, lanes with one counter combined first (two leader-and-ballot turns)
template <class Ptr>
__device__ __forceinline__ void count(Ptr counters, bool active, uint32_t bin, int lane) {
    uint64_t waiting = __ballot(active);
#pragma unroll
    for (int turn = 0; turn < 2; ++turn) {
        if (!waiting) break;
        const int leader = __ffsll((long long)waiting) - 1;
        const uint32_t lbin = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
        const uint64_t same = __ballot(active && bin == lbin) & waiting;
        if (lane == leader) atomicAdd(&counters[lbin], (uint32_t)__popcll(same));
        waiting &= ~same;
    }
    if ((waiting >> lane) & 1ull) atomicAdd(&counters[bin], 1u);
}

// pass 0 (prefix < 0): the top digit of every row; pass 1: the low digit of the rows whose top digit is `prefix`
__global__ __launch_bounds__(kThreads) void lds8_kernel(const uint16_t* keys, int64_t n, int prefix, uint32_t* hist) {
    __shared__ uint32_t lh[256];
    const int tid = threadIdx.x, lane = tid & 63;
    lh[tid] = 0;
    __syncthreads();
    const int64_t ntiles = (n + kTile - 1) / kTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
        for (int b = 0; b < kPer / kBatch; ++b) {
            uint32_t key[kBatch];
            bool in[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int64_t row = tile * kTile + (int64_t)(b * kBatch + k) * kThreads + tid;
                in[k] = row < n;
                key[k] = keys[in[k] ? row : n - 1];
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const bool active = in[k] && (prefix < 0 || (int)(key[k] >> 8) == prefix);
                count(lh, active, prefix < 0 ? key[k] >> 8 : key[k] & 255u, lane);
            }
        }
    __syncthreads();
    if (lh[tid]) atomicAdd(&hist[tid], lh[tid]);
}

__global__ __launch_bounds__(kThreads) void global16_kernel(const uint16_t* keys, int64_t n, uint32_t* hist) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t ntiles = (n + kTile - 1) / kTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
        for (int b = 0; b < kPer / kBatch; ++b) {
            uint32_t key[kBatch];
            bool in[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int64_t row = tile * kTile + (int64_t)(b * kBatch + k) * kThreads + tid;
                in[k] = row < n;
                key[k] = keys[in[k] ? row : n - 1];
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) count(hist, in[k], key[k], lane);
        }
}

static int bucket_of(const std::vector<uint32_t>& h, uint64_t& rank) {
    for (size_t b = 0; b < h.size(); ++b) {
        if (rank < h[b]) return (int)b;
        rank -= h[b];
    }
    return (int)h.size() - 1;
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? (int64_t)atof(argv[1]) : 50000000;
    const int reps = argc > 2 ? atoi(argv[2]) : 5;
    if (n < 1 || reps < 1) { fprintf(stderr, "usage: %s [rows] [reps]\n", argv[0]); return 2; }
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int64_t ntiles = (n + kTile - 1) / kTile;
    const int grid = (int)(ntiles < (int64_t)prop.multiProcessorCount * 8 ? ntiles : (int64_t)prop.multiProcessorCount * 8);
    uint16_t* keys;
    uint32_t* hist;
    CK(hipMalloc(&keys, (size_t)n * 2));
    CK(hipMalloc(&hist, 65536 * 4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const char* names[] = {"uniform", "equal", "two"};
    for (int kind = 0; kind < 3; ++kind) {
        hipLaunchKernelGGL(fill_kernel, dim3(grid), dim3(kThreads), 0, 0, keys, n, kind);
        CK(hipDeviceSynchronize());
        const uint64_t median = (uint64_t)(n - 1) / 2;
        int key_a = -1, key_b = -1;
        float best_a = 1e30f, best_b = 1e30f;
        std::vector<uint32_t> h256(256), h64k(65536);
        for (int r = 0; r <= reps; ++r) {          // (the first repetition is not counted)
            // ---- two LDS passes; the bucket of the median comes back between them (the library plans it on the device: one
            // more launch of one block, not a host round trip), so each pass is timed on its own and the two are added
            float ms0 = 0, ms1 = 0;
            CK(hipMemset(hist, 0, 65536 * 4));
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(lds8_kernel, dim3(grid), dim3(kThreads), 0, 0, keys, n, -1, hist);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms0, e0, e1));
            CK(hipMemcpy(h256.data(), hist, 256 * 4, hipMemcpyDeviceToHost));
            uint64_t rank = median;
            const int top = bucket_of(h256, rank);
            CK(hipMemset(hist, 0, 65536 * 4));
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(lds8_kernel, dim3(grid), dim3(kThreads), 0, 0, keys, n, top, hist);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms1, e0, e1));
            CK(hipMemcpy(h256.data(), hist, 256 * 4, hipMemcpyDeviceToHost));
            key_a = top * 256 + bucket_of(h256, rank);
            if (r > 0 && ms0 + ms1 < best_a) best_a = ms0 + ms1;
            // ---- one pass into global counters
            float ms = 0;
            CK(hipMemset(hist, 0, 65536 * 4));
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(global16_kernel, dim3(grid), dim3(kThreads), 0, 0, keys, n, hist);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(h64k.data(), hist, 65536 * 4, hipMemcpyDeviceToHost));
            rank = median;
            key_b = bucket_of(h64k, rank);
            if (r > 0 && ms < best_b) best_b = ms;
        }
        printf("{\"op\": \"hist16\", \"rows\": %lld, \"column\": \"%s\", \"lds8x2_ms\": %.4f, \"global16_ms\": %.4f, \"global16_over_lds8x2\": %.2f, \"median_key\": %d, \"agree\": %s}\n",
               (long long)n, names[kind], best_a, best_b, best_b / best_a, key_a, key_a == key_b ? "true" : "false");
        if (key_a != key_b) return 1;
    }
    return 0;
}
