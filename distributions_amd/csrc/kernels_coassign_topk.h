// Held-out rows: per query, the k targets it is most likely co-assigned with
// over M engines, without the dense matrix.  Part of
// kernels.h, after kernels_coassign.h.
//
// cell(a, b) is bit for bit what k_coassign_gemm writes for the same rows: the
// same contraction (coassign_contract), the same division.  Targets are
// ordered by
//   key = (uint64(bits(cell)) << 32) | (0xFFFFFFFF - b),  descending:
// cells of specified rows are >= +0 and never NaN, so their bits order as the
// floats do, and among bit-equal cells the smaller b comes first.  Keys of
// distinct targets are distinct (b <= 2^32 - 2: the low word is >= 1), so the
// k largest keys of a row are the same whatever the tiles, chunks and launch
// geometry.  Key 0 is "no target": below every real key, and decoded as index
// 0xFFFFFFFF with +0.0f.
//
// k_coassign_topk       a tile's cells, then per row of the tile its kc
//                       largest keys, descending, into the candidate array;
//                       where the targets are the queries also per COLUMN of a
//                       tile off the diagonal, for the rows that its mirror
//                       would have held (the cells are their own transposes)
// k_coassign_topk_merge a query row's running k keys with the row's
//                       candidates of one launch -> the k largest
// k_coassign_topk_decode  keys -> index_out, prob_out
#pragma once

namespace dist {

// a tile parked in LDS: 129 words a row, so that the lanes of a wave that
// walk 64 rows at one column, or 64 columns at one row, meet 64 banks
constexpr int kCoTopkRow = kCoTile + 1;
// the word of a masked cell (a NaN: no specified cell has it)
constexpr uint32_t kCoTopkMasked = 0xFFFFFFFFu;

struct CoassignTopk {
    const PredictMember * q;
    const PredictMember * t;
    int m;
    int sym;             // as CoassignGemm's: a block on the call's diagonal
    int exclude;         // the cell whose row is its column is left out
    int kc;              // keys per (row, tile): min(k, kCoTile)
    size_t ldq, ldt;
    size_t n_q, n_t;     // the launch's rows and columns
    size_t q0, t0;       // the call's index of the launch's first row / column
    unsigned tiles_q, tiles_t;
    // [row of the launch][tile of its columns][kc]
    unsigned long long * cand_q;
    // the targets are the queries: [column of the launch][tile of its
    // rows][kc], what the block's transpose would have given its rows; sym:
    // cand_t == cand_q (a tile on the diagonal holds both); else null
    unsigned long long * cand_t;
    float fm;            // (float) of the CALL's m
};
// dynamic LDS of k_coassign_topk: the slabs of the contraction, then the
// tile in their place (more than kLdsNoOptIn: the launch opts in)
constexpr size_t coassign_topk_lds() {
    const size_t tile = (size_t)kCoTile * kCoTopkRow * sizeof(uint32_t);
    return tile > coassign_gemm_lds() ? tile : coassign_gemm_lds();
}

// One line of a parked tile (a row: stride 1, a column: stride kCoTopkRow):
// its kc largest keys in descending order -> out[0..kc).  low0 is the low word
// of the line's first cell, 0xFFFFFFFF - (its target's index in the call).
// Round j takes the largest key below round j - 1's: the keys are distinct.
__device__ __forceinline__ void coassign_topk_line(
        const uint32_t * line, int stride, uint32_t low0, int kc,
        unsigned long long * out) {
    unsigned long long prev = ~0ull;
    int j = 0;
    for (; j < kc; ++j) {
        unsigned long long best = 0;
#pragma unroll 8
        for (int c = 0; c < kCoTile; ++c) {
            const uint32_t w = line[c * stride];
            const unsigned long long key =
                w == kCoTopkMasked
                    ? 0ull
                    : ((unsigned long long)w << 32) | (low0 - (uint32_t)c);
            if (key < prev && key > best) best = key;
        }
        if (best == 0) break;
        out[j] = best;
        prev = best;
    }
    for (; j < kc; ++j) out[j] = 0;
}

// k_coassign_gemm's tiling and loop; the epilogue divides, masks (columns >=
// n_t, rows >= n_q, the excluded self cell) and parks the tile in LDS, then
// threads 0-127 take a row each and, where the columns are wanted, threads
// 128-255 a column each.
__global__ __launch_bounds__(kBlock) void k_coassign_topk(CoassignTopk G) {
    extern __shared__ float co_lds[];
    const unsigned it = blockIdx.y, jt = blockIdx.x;
    if (G.sym && jt < it) return;
    const size_t i0 = (size_t)it * kCoTile, j0 = (size_t)jt * kCoTile;
    co_f32x16 acc[2][2];
    const CoassignLane L = coassign_contract(G.q, G.t, G.m, G.ldq, G.ldt, it,
                                             jt, co_lds, acc);
    uint32_t * const tile = reinterpret_cast<uint32_t *>(co_lds);
    __syncthreads();     // (the last slab has been read)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const unsigned col = L.wj + b * 32 + L.oc;
            const size_t j = j0 + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned row =
                    L.wi + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * L.ok;
                const size_t i = i0 + row;
                const bool live = i < G.n_q && j < G.n_t
                    && !(G.exclude && G.q0 + i == G.t0 + j);
                tile[row * kCoTopkRow + col] =
                    live ? __float_as_uint(acc[a][b][r] / G.fm)
                         : kCoTopkMasked;
            }
        }
    __syncthreads();
    const unsigned line = threadIdx.x & (kCoTile - 1);
    if (threadIdx.x < kCoTile) {
        const size_t i = i0 + line;
        if (i < G.n_q)
            coassign_topk_line(
                tile + line * kCoTopkRow, 1, ~(uint32_t)(G.t0 + j0), G.kc,
                G.cand_q + (i * G.tiles_t + jt) * (size_t)G.kc);
    } else if (G.cand_t != nullptr && !(G.sym && jt == it)) {
        const size_t j = j0 + line;
        if (j < G.n_t)
            coassign_topk_line(
                tile + line, kCoTopkRow, ~(uint32_t)(G.q0 + i0), G.kc,
                G.cand_t + (j * G.tiles_q + it) * (size_t)G.kc);
    }
}

// the largest of a wave's 64 keys, in every lane
__device__ __forceinline__ unsigned long long coassign_wave_max(
        unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One query row per workgroup of one wave: run[row][0..k) (descending, key 0
// last) merged with the row's `tiles` candidate lists of kc keys each
// (cand[row][tile][kc], each descending) -> run[row], the k largest.  Lists
// are taken 64 at a time, one per lane: a round picks the largest head among
// the lanes' lists and the running list, and whoever held it moves on.
constexpr int kCoTopkMergeBlock = 64;
__global__ __launch_bounds__(kCoTopkMergeBlock) void k_coassign_topk_merge(
        const unsigned long long * __restrict__ cand, unsigned tiles, int kc,
        int k, unsigned long long * __restrict__ run) {
    __shared__ unsigned long long s_run[kCoTile];
    const int lane = (int)threadIdx.x;
    const size_t row = blockIdx.x;
    unsigned long long * const mine = run + row * (size_t)k;
    for (int j = lane; j < k; j += kCoTopkMergeBlock) s_run[j] = mine[j];
    __syncthreads();
    const unsigned long long * const lists = cand + row * tiles * (size_t)kc;
    for (unsigned g0 = 0; g0 < tiles; g0 += kCoTopkMergeBlock) {
        const unsigned long long * const list =
            g0 + lane < tiles ? lists + (size_t)(g0 + lane) * kc : nullptr;
        int at = 0, run_at = 0;
        unsigned long long head = list ? list[0] : 0ull;
        unsigned long long run_head = s_run[0];
        unsigned long long o0 = 0, o1 = 0;
        for (int j = 0; j < k; ++j) {
            const unsigned long long lanes = coassign_wave_max(head);
            const unsigned long long best = run_head > lanes ? run_head : lanes;
            if (best == 0) break;              // (the whole wave: no key left)
            if (run_head > lanes) {
                ++run_at;
                run_head = run_at < k ? s_run[run_at] : 0ull;
            } else if (head == lanes) {        // (one lane: keys are distinct)
                ++at;
                head = at < kc ? list[at] : 0ull;
            }
            if (lane == (j & 63)) {
                if (j < 64) o0 = best;
                else o1 = best;
            }
        }
        __syncthreads();
        if (lane < k) s_run[lane] = o0;
        if (lane + 64 < k) s_run[lane + 64] = o1;
        __syncthreads();
    }
    for (int j = lane; j < k; j += kCoTopkMergeBlock) mine[j] = s_run[j];
}

// run[a][j] -> index_out[a * ld + j] = 0xFFFFFFFF - low word, prob_out = the
// high word's float; key 0 is 0xFFFFFFFF and +0.0f
__global__ __launch_bounds__(kBlock) void k_coassign_topk_decode(
        const unsigned long long * __restrict__ run, size_t n_q, int k,
        uint32_t * __restrict__ index_out, float * __restrict__ prob_out,
        size_t ld) {
    const size_t at = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (at >= n_q * (size_t)k) return;
    const size_t a = at / (size_t)k, j = at % (size_t)k;
    const unsigned long long key = run[at];
    index_out[a * ld + j] = ~(uint32_t)key;
    prob_out[a * ld + j] = __uint_as_float((uint32_t)(key >> 32));
}

}  // namespace dist
