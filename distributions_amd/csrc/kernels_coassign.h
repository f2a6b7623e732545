// Held-out rows: co-assignment of row pairs over M engines, on the matrix
// cores.  Part of kernels.h.
//
// For engine e and row a, scores[k], m and total are k_predict's passes 1 and
// 2 (kernels_predict.h; scores_to_likelihoods, random.cc:94-103), empty groups
// included.  Then
//   r_e,a[k]  = fast_exp(scores[k] - m) * (1.0f / total): one IEEE float
//               division per row, one float multiply per group, subnormal
//               results flushed to zero (the build's
//               -fgpu-flush-denormals-to-zero).  The normalisation is per
//               engine, so LowEntropy needs nothing more;
//   acc[a][b] = fmaf(r_e,a[k], r_e,b[k], acc[a][b]) from 0.0f, ONE chain per
//               cell: engines ascending, k ascending within an engine; no
//               split over k, no second accumulator, padding entries exact
//               zeros (fmaf(0, 0, acc) == acc for acc >= +0);
//   out[a*ld + b] = acc[a][b] / (float)m, IEEE division.
// Phase A (k_coassign_resp) writes r as k-major planes W_e[k][row]; phase B
// (k_coassign_gemm) contracts them with v_mfma_f32_32x32x2_f32, whose result
// is bit for bit the k-ordered fmaf chain (one rounding per product, the
// accumulator never flushed).
#pragma once

namespace dist {

// The GEMM's tile of `out` (rows x columns) and the k rows of a plane that
// are staged at a time.  Planes are padded to kCoTile rows and an even k.
constexpr int kCoTile = 128;
constexpr int kCoSlab = 32;
// a staged k row: kCoTile floats and half a row of banks, so that the two
// k rows an MFMA operand reads (lanes 0-31, lanes 32-63) meet no bank twice
constexpr int kCoRow = kCoTile + 32;
constexpr size_t coassign_pad_rows(size_t rows) {
    return (rows + kCoTile - 1) / kCoTile * kCoTile;
}
constexpr int coassign_pad_k(int k) { return (k + 1) & ~1; }

// Phase A: k_predict's passes 1 and 2 for every (member, row), then a third
// pass that writes r[k]; grid (row blocks over rows_pad, M), one lane per row.
// The member's plane is its A.logp: r[k] of row q at plane[k * ld + q],
// consecutive lanes consecutive words.  Rows in [P.row_end, rows_pad) and,
// with pad_k, the row k = K of an odd K are written as zeros: the GEMM loads
// whole tiles of an even number of k rows without guards.
template <int KIND0, int KIND1, int NF>
__global__ __launch_bounds__(kBlock) void k_coassign_resp(
        const PredictMember * __restrict__ all, size_t ld, size_t rows_pad,
        int pad_k) {
    __shared__ uint32_t s_exp[1024];
    predict_load_exp(s_exp);
    const PredictMember & M = all[blockIdx.y];
    const SweepParams & P = M.P;
    const PredictArgs & A = M.A;
    const float ea = u2f(g_tables_dev.exp_ab[0]);
    const float eb = u2f(g_tables_dev.exp_ab[1]);
    const int K = P.K;
    const size_t q = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= rows_pad) return;
    const bool live = q < P.row_end;
    const PredictScorer<KIND0, KIND1, NF> ps(P, A, live ? q : 0, live);
    // vector_max (vector_math.cc:74-83)
    float m = ps.at(0);
#pragma unroll kSweepUnroll
    for (int k = 1; k < K; ++k) {
        const float s = ps.at(k);
        m = s > m ? s : m;
    }
    float total = 0.f;
#pragma unroll kSweepUnroll
    for (int k = 0; k < K; ++k)
        total += fast_exp_nonpos(ps.at(k) - m, s_exp, ea, eb);
    const float inv = 1.0f / total;
    float * const w = A.logp + q;
#pragma unroll kSweepUnroll
    for (int k = 0; k < K; ++k) {
        const float r = fast_exp_nonpos(ps.at(k) - m, s_exp, ea, eb) * inv;
        w[(size_t)k * ld] = live ? r : 0.f;
    }
    if (pad_k && (K & 1)) w[(size_t)K * ld] = 0.f;
}

// Phase B.  q and t are the members' arrays of the query and of the target
// launch of phase A (the same array when the targets are the queries): member
// e's planes are q[e].A.logp [K2_e][ldq] and t[e].A.logp [K2_e][ldt], K2_e =
// coassign_pad_k(q[e].P.K).
struct CoassignGemm {
    const PredictMember * q;
    const PredictMember * t;
    int m;
    int sym;             // 1: t == q (a block on the call's diagonal): tiles
                         // below the block's diagonal are not computed
    size_t ldq, ldt;
    size_t n_q, n_t;     // the launch's rows and columns of `out`
    float * out;         // the launch's first cell
    // the first cell of the block's transpose in the call's output, or null:
    // cell (i, j) is also written at mirror[j * ld + i] (the targets are the
    // queries; sym: mirror == out, and a tile on the diagonal holds both)
    float * mirror;
    size_t ld;
    float fm;            // (float) of the CALL's m
};
// dynamic LDS of k_coassign_gemm: a slab of each operand
constexpr size_t coassign_gemm_lds() {
    return (size_t)2 * kCoSlab * kCoRow * sizeof(float);
}

// A workgroup of four waves owns a kCoTile x kCoTile tile of `out`, wave w
// the 64 x 64 quarter (w >> 1, w & 1) as 2 x 2 sub-tiles of 32 x 32: sixteen
// accumulator registers per sub-tile, ONE accumulator per cell for the whole
// call.  The loop over the members runs in here; per member, slabs of
// kCoSlab k rows of both planes go through LDS (k-major planes: global and
// LDS reads are contiguous), two k per MFMA, k ascending.
// Operands (32x32x2): lane l holds A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; D: column = lane & 31, row = (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5).  Loads are unguarded (padded planes).
typedef float co_f32x16 __attribute__((ext_vector_type(16)));
// what a thread is in its tile
struct CoassignLane {
    unsigned wi, wj;     // its wave's quarter: first row and column
    unsigned ok, oc;     // operands: the k row within a pair and the row /
                         // column of a sub-tile
};
// The contraction of tile (it, jt) of the launch, shared by k_coassign_gemm
// and k_coassign_topk (kernels_coassign_topk.h): -> acc, the cells' chains
// before the division.  co_lds: coassign_gemm_lds() bytes.  Ends after the
// last MFMA's operand reads, without a barrier.
__device__ __forceinline__ CoassignLane coassign_contract(
        const PredictMember * q, const PredictMember * t, int m, size_t ldq,
        size_t ldt, unsigned it, unsigned jt, float * co_lds,
        co_f32x16 (&acc)[2][2]) {
    float * const sA = co_lds;
    float * const sB = co_lds + kCoSlab * kCoRow;
    const unsigned tid = threadIdx.x;
    const unsigned lane = tid & 63u, wave = tid >> 6;
    const unsigned wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const size_t i0 = (size_t)it * kCoTile, j0 = (size_t)jt * kCoTile;
    // staging: 32 threads copy one k row of a tile, four floats each
    const unsigned lr = tid >> 5, lc = (tid & 31u) * 4;
    const unsigned ok = lane >> 5, oc = lane & 31u;

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    for (int e = 0; e < m; ++e) {
        const int K2 = coassign_pad_k(q[e].P.K);
        const float * const pa = q[e].A.logp + i0 + lc;
        const float * const pb = t[e].A.logp + j0 + lc;
        for (int k0 = 0; k0 < K2; k0 += kCoSlab) {
            const int h = K2 - k0 < kCoSlab ? K2 - k0 : kCoSlab;   // (even)
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kCoSlab; r += kBlock / 32) {
                const int kr = r + (int)lr;
                if (kr < h) {
                    const float4 va = *reinterpret_cast<const float4 *>(
                        pa + (size_t)(k0 + kr) * ldq);
                    const float4 vb = *reinterpret_cast<const float4 *>(
                        pb + (size_t)(k0 + kr) * ldt);
                    *reinterpret_cast<float4 *>(sA + kr * kCoRow + lc) = va;
                    *reinterpret_cast<float4 *>(sB + kr * kCoRow + lc) = vb;
                }
            }
            __syncthreads();
            for (int kk = 0; kk < h; kk += 2) {
                const float * const ra = sA + (kk + ok) * kCoRow + wi + oc;
                const float * const rb = sB + (kk + ok) * kCoRow + wj + oc;
                const float a0 = ra[0], a1 = ra[32];
                const float b0 = rb[0], b1 = rb[32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                    a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                    a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                    a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                    a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    return CoassignLane{wi, wj, ok, oc};
}

// The dense form: the stores are guarded by n_q and n_t.
__global__ __launch_bounds__(kBlock) void k_coassign_gemm(CoassignGemm G) {
    extern __shared__ float co_lds[];
    const unsigned it = blockIdx.y, jt = blockIdx.x;
    if (G.sym && jt < it) return;
    const size_t i0 = (size_t)it * kCoTile, j0 = (size_t)jt * kCoTile;
    co_f32x16 acc[2][2];
    const CoassignLane L = coassign_contract(G.q, G.t, G.m, G.ldq, G.ldt, it,
                                             jt, co_lds, acc);
    const unsigned wi = L.wi, wj = L.wj, ok = L.ok, oc = L.oc;

    const bool mirror = G.mirror != nullptr && !(G.sym && jt == it);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const size_t j = j0 + wj + b * 32 + oc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const size_t i =
                    i0 + wi + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * ok;
                if (i < G.n_q && j < G.n_t) {
                    const float v = acc[a][b][r] / G.fm;
                    G.out[i * G.ld + j] = v;
                    // (the transposed block: n_t rows of n_q cells)
                    if (mirror) G.mirror[j * G.ld + i] = v;
                }
            }
        }
}

}  // namespace dist
