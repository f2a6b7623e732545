// Agreement of P partitions of the same N rows (dist_partition_agreement_dev,
// dist_gibbs_partition_agreement_many) and the co-assignment of resident rows
// over M engines (dist_gibbs_coassign_resident_many).  DESIGN 4.22.
//
// For partitions a, b with contingency cells n_gh the calls need
//   sq[a][b]    = sum n_gh^2               (uint64, exact in any order)
//   nlogn[a][b] = sum n_gh log(n_gh)       (binary64, fixed order)
// and nothing else; the N x N similarity matrix is never formed.  Per a the
// rows are sorted stably by a's label (k_cs_hist / k_cs_scan / k_cs_scatter of
// kernels_apply.h as they are, or the library radix sort past kCsMaxKeys),
// then ONE launch of k_partition_pairs covers every b >= a: scratch is the N
// words of the order and K_a + 2 offsets.
#pragma once

namespace dist {

// A partition as the kernels read it: a column of n_rows words; an engine's
// holds global group ids, which g2p (n_global entries, -1 = retired) turns into
// packed indices; a caller's column is its own bins (g2p == nullptr).
struct PartitionCol {
    const uint32_t * labels;
    const int32_t * g2p;
    uint32_t n_global;
    uint32_t n_labels;   // exclusive bound on the bins
};

constexpr uint32_t kPartitionNoBin = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t partition_bin(const PartitionCol & c,
                                                  size_t row) {
    const uint32_t id = c.labels[row];
    if (c.g2p == nullptr) return id < c.n_labels ? id : kPartitionNoBin;
    if (id >= c.n_global) return kPartitionNoBin;
    const int32_t p = c.g2p[id];
    return p >= 0 && (uint32_t)p < c.n_labels ? (uint32_t)p : kPartitionNoBin;
}

// bad[c] = the first row of column c whose label has no bin (~0: none).  Runs
// before anything else reads a label; the call stops there if one is found.
__global__ __launch_bounds__(kBlock) void k_partition_check(
        const PartitionCol * __restrict__ cols, size_t n_rows,
        unsigned long long * __restrict__ bad) {
    const PartitionCol c = cols[blockIdx.y];
    unsigned long long first = ~0ull;
    for (size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x; row < n_rows;
         row += (size_t)gridDim.x * kBlock)
        if (partition_bin(c, row) == kPartitionNoBin) {
            first = row;
            break;
        }
    if (first != ~0ull) atomicMin(bad + blockIdx.y, first);
}

// an engine's column as bins, the form the counting sort takes its keys in
__global__ __launch_bounds__(kBlock) void k_partition_keys(
        const PartitionCol * __restrict__ cols, int a, size_t n_rows,
        uint32_t * __restrict__ keys) {
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row < n_rows) keys[row] = partition_bin(cols[a], row);
}

// the radix route's values: row e travels as 2 e + 1, k_cs_scatter's
// convention for additions, so that both routes leave the same order[]
__global__ __launch_bounds__(kBlock) void k_partition_iota(
        size_t n_rows, uint32_t * __restrict__ vals) {
    const size_t row = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (row < n_rows) vals[row] = (uint32_t)(2 * row + 1);
}

// ... and its offsets: offset[k] = the sorted keys below k, k in [0, n_keys]
__global__ __launch_bounds__(kBlock) void k_partition_offsets(
        const uint32_t * __restrict__ keys_sorted, size_t n_rows, int n_keys,
        uint32_t * __restrict__ offset) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k > n_keys) return;
    size_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (keys_sorted[mid] < (uint32_t)k) lo = mid + 1; else hi = mid;
    }
    offset[k] = (uint32_t)lo;
}

// k_partition_pairs: workgroup (x, y) walks the segments g = x, x + gridDim.x,
// ... of partition a against partition b = b0 + y.  Its LDS holds one uint32
// bin and one uint32 "first position" per label of b, cleared once; per
// segment
//   walk 1  bins[l] += 1 (LDS atomic); the lane that found the bin empty
//           resets first[l]
//   walk 2  first[l] = min(first[l], position): the cell's first row in the
//           (stable) order, whoever won walk 1
//   walk 3  sum += bins[l] -- the sum over a cell's rows of its size is its
//           square, so no pass over K_b bins is needed -- and the cell's first
//           row adds n log n
//   walk 4  bins[l] = 0: only the bins that were touched
// so a pair costs O(N) whatever K_a K_b is.  Without nlogn walk 2 and the
// first[] half are skipped.  Sums are uint64 from the first add (one group of
// 70 000 rows has n^2 > 2^32); the workgroup's total goes to sq with one 64-bit
// integer atomic, exact in any order.  The binary64 partial of a workgroup --
// its threads' sums over their rows in segment order, then a fixed tree --
// goes to part[y * gridDim.x + x]; k_partition_nlogn adds them in x order.
// The grid is a function of (K_a, P - a) alone, so equal calls give equal
// bits.
constexpr size_t partition_pairs_lds(size_t bins) { return bins * 8; }
// the bin limit: what partition_pairs_lds allows under kLdsWorkgroupLimit
constexpr size_t kPartitionMaxBins = kLdsWorkgroupLimit / 8;   // 18 432
static_assert(partition_pairs_lds(kPartitionMaxBins) <= kLdsWorkgroupLimit
                  && partition_pairs_lds(kPartitionMaxBins + 1)
                         > kLdsWorkgroupLimit,
              "the bin limit is the formula's");

struct PartitionPairs {
    const PartitionCol * cols;
    const uint32_t * order;     // [n_rows] 2 row + 1, sorted by a's bin
    const uint32_t * offset;    // [K_a + 1]
    unsigned long long * sq;    // [P][P]
    double * part;              // [gridDim.y][gridDim.x] or nullptr
    int p;
    int a;
    int b0;
    int k_a;
    uint32_t lds_bins;          // first[] begins here
};

__global__ __launch_bounds__(kBlock) void k_partition_pairs(PartitionPairs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pp_lds[];
    __shared__ unsigned long long s_sq[kBlock / 64];
    __shared__ double s_nl[kBlock / 64];
    const int b = A.b0 + (int)blockIdx.y;
    const PartitionCol cb = A.cols[b];
    const bool want_nl = A.part != nullptr;
    uint32_t * bins = pp_lds;
    uint32_t * first = pp_lds + A.lds_bins;
    for (uint32_t k = threadIdx.x; k < cb.n_labels; k += kBlock) bins[k] = 0;
    __syncthreads();
    unsigned long long sum = 0;
    double nl = 0.0;
    for (int g = (int)blockIdx.x; g < A.k_a; g += (int)gridDim.x) {
        const uint32_t begin = A.offset[g], end = A.offset[g + 1];
        if (begin == end) continue;   // (uniform: no barrier is skipped by some)
        for (uint32_t i = begin + threadIdx.x; i < end; i += kBlock) {
            const uint32_t l = partition_bin(cb, A.order[i] >> 1);
            if (l == kPartitionNoBin) continue;
            if (atomicAdd(&bins[l], 1u) == 0u && want_nl)
                first[l] = 0xFFFFFFFFu;
        }
        __syncthreads();
        if (want_nl) {
            for (uint32_t i = begin + threadIdx.x; i < end; i += kBlock) {
                const uint32_t l = partition_bin(cb, A.order[i] >> 1);
                if (l != kPartitionNoBin) atomicMin(&first[l], i);
            }
            __syncthreads();
        }
        for (uint32_t i = begin + threadIdx.x; i < end; i += kBlock) {
            const uint32_t l = partition_bin(cb, A.order[i] >> 1);
            if (l == kPartitionNoBin) continue;
            const uint32_t n = bins[l];
            sum += n;
            if (want_nl && first[l] == i && n > 1u)
                nl += (double)n * log((double)n);
        }
        __syncthreads();
        for (uint32_t i = begin + threadIdx.x; i < end; i += kBlock) {
            const uint32_t l = partition_bin(cb, A.order[i] >> 1);
            if (l != kPartitionNoBin) bins[l] = 0;
        }
        __syncthreads();
    }
    // the workgroup's totals: a fixed tree over the lanes, the waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        nl += __shfl_down(nl, off);
    }
    if (lane == 0) {
        s_sq[wave] = sum;
        s_nl[wave] = nl;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long total = 0;
    double total_nl = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) {
        total += s_sq[w];
        total_nl += s_nl[w];
    }
    if (total) {
        atomicAdd(A.sq + (size_t)A.a * A.p + b, total);
        if (b != A.a) atomicAdd(A.sq + (size_t)b * A.p + A.a, total);
    }
    if (want_nl) A.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total_nl;
}

// nlogn[a][b] and its mirror: the workgroups' partials in x order
__global__ __launch_bounds__(kBlock) void k_partition_nlogn(
        const double * __restrict__ part, int groups, int n_b, int p, int a,
        int b0, double * __restrict__ nlogn) {
    const int y = blockIdx.x * kBlock + threadIdx.x;
    if (y >= n_b) return;
    double s = 0.0;
    for (int x = 0; x < groups; ++x) s += part[(size_t)y * groups + x];
    const int b = b0 + y;
    nlogn[(size_t)a * p + b] = s;
    nlogn[(size_t)b * p + a] = s;
}

// out[i][j] = (the engines in which resident rows rows_a[i] and rows_b[j]
// carry the same group id) / m: a thread per cell, a loop over the engines.
// Global ids of one engine compare as they are.
__global__ __launch_bounds__(kBlock) void k_coassign_resident(
        const uint32_t * const * __restrict__ assign, int m,
        const uint32_t * __restrict__ rows_a, size_t na,
        const uint32_t * __restrict__ rows_b, size_t nb, size_t n_rows,
        float * __restrict__ out, size_t ld) {
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= na * nb) return;
    const size_t i = cell / nb, j = cell % nb;
    const uint32_t ra = rows_a[i], rb = rows_b[j];
    // (k_partition_rows_check reports such an index; nothing is read there)
    if (ra >= n_rows || rb >= n_rows) return;
    uint32_t c = 0;
    for (int e = 0; e < m; ++e) {
        const uint32_t * col = assign[e];
        c += col[ra] == col[rb] ? 1u : 0u;
    }
    out[i * ld + j] = (float)c / (float)m;
}

// rows[i] >= n_rows: the first such index to bad (~0: none)
__global__ __launch_bounds__(kBlock) void k_partition_rows_check(
        const uint32_t * __restrict__ rows, size_t n, size_t n_rows,
        unsigned long long * __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n && rows[i] >= n_rows) atomicMin(bad, (unsigned long long)i);
}

}  // namespace dist
