// Resident rows: per query the k rows of the table it is most co-assigned with
// over M engines, without the [n_q, N] matrix.  Part of
// kernels.h, after kernels_partitions.h.
//
// The targets are the engines' resident rows b in [row_begin, row_end).  Two
// kinds of query:
//   held-out  rows that are not in the table, given as values.  With r_e,q[k]
//             bit for bit dist_gibbs_responsibilities' value (phase A of
//             kernels_coassign.h, k-major planes W_e[k][q]) and
//             slot_e(b) = g2p_e[assign_e[b]] (partition_bin),
//               acc = 0.0f; engines ascending: acc = acc + r_e,q[slot_e(b)]
//               cell(q, b) = acc / (float)m
//             one chain of binary32 adds: no product, nothing to contract.
//   resident  rows of the table, given as indices.  cell(a, b) = (float)c /
//             (float)m with c the engines in which rows[a] and b carry the
//             same global id: k_coassign_resident's cell.  The kernel selects
//             on (c, b) -- (float)c / (float)m grows strictly with c for c <=
//             m <= 65535 -- and makes the float once, at the end.
// Order and fill are kernels_coassign_topk.h's: key = (bits(cell) << 32) |
// (0xFFFFFFFF - b) descending, key 0 "no target".  The candidates are written
// as cand[query][slice][kc], k_coassign_topk_merge's input.
#pragma once

namespace dist {

// queries of a workgroup, and the targets of a tile (a thread each)
constexpr int kSearchQ = 16;
constexpr int kSearchTile = kBlock;
// a query's running list: 128 keys, two to a lane of the wave that owns it
constexpr int kSearchList = 128;
static_assert(kSearchList == kCoTile, "k is at most the merge's list");
static_assert(kSearchQ % (kBlock / 64) == 0, "queries divide over the waves");

struct ResidentTopk {
    const PartitionCol * cols;       // [m] the engines' labels and maps
    // held-out: member e's plane [K_e][ldq], the launch's queries
    const float * const * planes;
    size_t ldq;
    // resident: qlab[e * ldl + a] = assign_e[rows[a]]; rows: the launch's
    const uint32_t * qlab;
    size_t ldl;
    const uint32_t * rows;
    int m;
    int kc;                          // keys per (query, slice)
    int exclude;                     // resident: b == rows[a] is left out
    size_t n_q;                      // the launch's queries
    size_t t0, t1;                   // the launch's targets [t0, t1)
    size_t slice;                    // targets per slice
    unsigned slices;
    unsigned long long * cand;       // [n_q][slices][kc]
    // held-out: the first (engine << 32 | row) whose label has no slot
    unsigned long long * bad;
    float fm;                        // (float) m
};

// resident queries' labels, once per launch: a thread per (engine, query)
__global__ __launch_bounds__(kBlock) void k_resident_query_labels(
        const PartitionCol * __restrict__ cols, int m,
        const uint32_t * __restrict__ rows, size_t n_q, size_t n_rows,
        uint32_t * __restrict__ qlab, size_t ldl) {
    const size_t at = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (at >= (size_t)m * ldl) return;
    const size_t e = at / ldl, a = at % ldl;
    // (k_partition_rows_check reports an index past the rows; a padding query
    // is never written out)
    const uint32_t row = a < n_q ? rows[a] : 0xFFFFFFFFu;
    qlab[at] = row < n_rows ? cols[e].labels[row] : 0xFFFFFFFFu;
}

// x into the wave's descending list (entry `lane` in lo, `lane + 64` in hi);
// the last entry falls out.  x differs from every entry.
__device__ __forceinline__ void search_insert(unsigned long long x, int lane,
                                              unsigned long long & lo,
                                              unsigned long long & hi) {
    const int pos = __popcll(__ballot(lo > x)) + __popcll(__ballot(hi > x));
    const unsigned long long up_lo = __shfl_up(lo, 1, 64);
    const unsigned long long up_hi = __shfl_up(hi, 1, 64);
    const unsigned long long last_lo = __shfl(lo, 63, 64);
    const unsigned long long prev_hi = lane == 0 ? last_lo : up_hi;
    lo = lane < pos ? lo : lane == pos ? x : up_lo;
    hi = lane + 64 < pos ? hi : lane + 64 == pos ? x : prev_hi;
}

// Workgroup (x, y): slice x of the targets against queries [16 y, 16 y + 16).
// Per tile a thread takes one target: its label per engine once, coalesced,
// and sixteen accumulators.  A cell whose key exceeds its query's threshold
// -- the kc-th key of the query's list, 0 until the list is full -- goes to the
// query's survivor buffer in LDS; then wave w drains the buffers of queries
// 4 w .. 4 w + 3 into their lists, which it keeps in registers for the whole
// slice.  A later target of a bit-equal cell has the smaller key, so ties never
// survive a full list.  The order survivors arrive in does not matter: keys
// are distinct, the list is the set's kc largest.
template <bool HELD_OUT>
__global__ __launch_bounds__(kBlock) void k_resident_topk(ResidentTopk A) {
    __shared__ unsigned long long s_buf[kSearchQ][kSearchTile];
    __shared__ unsigned long long s_thr[kSearchQ];
    __shared__ uint32_t s_cnt[kSearchQ];
    __shared__ uint32_t s_self[kSearchQ];
    constexpr int kPerWave = kSearchQ / (kBlock / 64);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t q0 = (size_t)blockIdx.y * kSearchQ;
    const size_t begin = A.t0 + (size_t)blockIdx.x * A.slice;
    const size_t end = begin + A.slice < A.t1 ? begin + A.slice : A.t1;
    if (threadIdx.x < kSearchQ) {
        s_thr[threadIdx.x] = 0;
        s_cnt[threadIdx.x] = 0;
        // (0xFFFFFFFF is no target's index)
        s_self[threadIdx.x] =
            !HELD_OUT && A.exclude && q0 + threadIdx.x < A.n_q
                ? A.rows[q0 + threadIdx.x] : 0xFFFFFFFFu;
    }
    unsigned long long lo[kPerWave], hi[kPerWave], thr[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) lo[i] = hi[i] = thr[i] = 0;
    __syncthreads();
    for (size_t b0 = begin; b0 < end; b0 += kSearchTile) {
        const size_t b = b0 + threadIdx.x;
        const bool live = b < end;
        uint32_t high[kSearchQ];
        if (HELD_OUT) {
            float acc[kSearchQ];
#pragma unroll
            for (int q = 0; q < kSearchQ; ++q) acc[q] = 0.0f;
            for (int e = 0; e < A.m; ++e) {
                if (!live) continue;
                const uint32_t slot = partition_bin(A.cols[e], b);
                if (slot == kPartitionNoBin) {
                    atomicMin(A.bad, ((unsigned long long)e << 32) | b);
                    continue;
                }
                // (planes are padded to whole blocks of queries and 16-byte
                // aligned: four words a load)
                const float4 * const w = reinterpret_cast<const float4 *>(
                    A.planes[e] + (size_t)slot * A.ldq + q0);
#pragma unroll
                for (int v = 0; v < kSearchQ / 4; ++v) {
                    const float4 r = w[v];
                    acc[4 * v + 0] = acc[4 * v + 0] + r.x;
                    acc[4 * v + 1] = acc[4 * v + 1] + r.y;
                    acc[4 * v + 2] = acc[4 * v + 2] + r.z;
                    acc[4 * v + 3] = acc[4 * v + 3] + r.w;
                }
            }
#pragma unroll
            for (int q = 0; q < kSearchQ; ++q)
                high[q] = __float_as_uint(acc[q] / A.fm);
        } else {
#pragma unroll
            for (int q = 0; q < kSearchQ; ++q) high[q] = 0;
            for (int e = 0; e < A.m; ++e) {
                const uint32_t mine =
                    live ? A.cols[e].labels[b] : 0xFFFFFFFFu;
                // (the same words in every lane)
                const uint32_t * const theirs =
                    A.qlab + (size_t)e * A.ldl + q0;
#pragma unroll
                for (int q = 0; q < kSearchQ; ++q)
                    high[q] += theirs[q] == mine ? 1u : 0u;
            }
        }
        if (live) {
            const uint32_t low = ~(uint32_t)b;
#pragma unroll
            for (int q = 0; q < kSearchQ; ++q) {
                const unsigned long long key =
                    ((unsigned long long)high[q] << 32) | low;
                if (key > s_thr[q] && (uint32_t)b != s_self[q])
                    s_buf[q][atomicAdd(&s_cnt[q], 1u)] = key;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) {
            const int q = wave * kPerWave + i;
            const uint32_t n = s_cnt[q];
            for (uint32_t s = 0; s < n; ++s) {
                const unsigned long long x = s_buf[q][s];
                if (x <= thr[i]) continue;   // (the wave as one)
                search_insert(x, lane, lo[i], hi[i]);
                thr[i] = __shfl((A.kc - 1) & 64 ? hi[i] : lo[i],
                                (A.kc - 1) & 63, 64);
            }
            if (lane == 0 && n) {
                s_cnt[q] = 0;
                s_thr[q] = thr[i];
            }
        }
        __syncthreads();
    }
    // the lists, descending and zero-filled; a resident key's count becomes
    // its cell here
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
        const size_t q = q0 + (size_t)(wave * kPerWave + i);
        if (q >= A.n_q) continue;
        unsigned long long * const out =
            A.cand + (q * A.slices + blockIdx.x) * (size_t)A.kc;
        unsigned long long keys[2] = {lo[i], hi[i]};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            unsigned long long key = keys[h];
            if (!HELD_OUT && key != 0) {
                const float cell = (float)(uint32_t)(key >> 32) / A.fm;
                key = ((unsigned long long)__float_as_uint(cell) << 32)
                    | (uint32_t)key;
            }
            if (lane + 64 * h < A.kc) out[lane + 64 * h] = key;
        }
    }
}

}  // namespace dist
