// ee_rows.hpp - the "one wavefront per logits row" expressions, each written once.
//
// ee_loss.hip, ee_head.hip, ee_apgd.hip, ee_fab.hip and ee_sqatk.hip promise each other's BITS: the cross-entropy gradient inside the head's
// backward is ee_ce_f32's, APGD's CE loss is ee_ce_f32's, `pred` of APGD and FAB is ee_topk_i64's first column.  The build keeps
// expressions as written (-ffp-contract=off -fno-fast-math), so the promise holds exactly when every kernel evaluates the same expression
// tree - these.  Operand order and parentheses here are part of the contract.
#pragma once
#include <math.h>

#include "ee_common.hpp"

namespace ee {

constexpr int kRowsPerBlock = kBlock / kWave;  // a 64-lane wavefront owns one row
static inline unsigned row_grid(int B) { return static_cast<unsigned>((B + kRowsPerBlock - 1) / kRowsPerBlock); }

// xor-butterflies: every lane ends with the result.  There is deliberately no float wave_sum: a float sum that should go through the
// double butterfly says so with a cast at the call site (fc_ce_grad_*), one that stays in float is written out where it is.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// max and log-sum-exp of one row, as log_softmax needs them:  logp_k = (z_k - mx) - lse.  fp32 exponentials summed in double.
__device__ __forceinline__ void row_stats(const float *__restrict__ z, int K, int lane, float &mx, float &lse) {
    float m = -INFINITY;
    for (int k = lane; k < K; k += kWave) m = fmaxf(m, z[k]);
    mx = wave_max(m);
    double s = 0.0;
    for (int k = lane; k < K; k += kWave) s += static_cast<double>(expf(z[k] - mx));
    s = wave_sum(s);
    lse = logf(static_cast<float>(s));
}

// d CrossEntropy / d z_k = (softmax_k - target_k) * gscale; ce_grad is the hard-label case
__device__ __forceinline__ float ce_grad_soft(float z, float mx, float lse, float target, float gscale) {
    return (expf((z - mx) - lse) - target) * gscale;
}
__device__ __forceinline__ float ce_grad(float z, float mx, float lse, bool is_label, float gscale) {
    return ce_grad_soft(z, mx, lse, is_label ? 1.0f : 0.0f, gscale);
}

// the order of ee_topk_i64: by value descending, ties to the lower index, NaN above everything (as torch.topk)
__device__ __forceinline__ bool better(float va, int ia, float vb, int ib) {
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return na;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}

constexpr int kNone = 0x7fffffff;

// the best class of one row in that order among those not in taken[0 .. j) (every lane gets it), its logit in `val`;
// WANT_NAN: `nan` says whether one of the classes looked at holds a NaN
template <int M, bool WANT_NAN = false>
__device__ __forceinline__ int row_next(const float *__restrict__ z, int K, int lane, const int (&taken)[M], int j, float &val,
                                        bool *nan = nullptr) {
    float bv = 0.0f;
    int bi = kNone;
    [[maybe_unused]] int any = 0;
    for (int c = lane; c < K; c += kWave) {
        bool skip = false;
#pragma unroll
        for (int jj = 0; jj < M; ++jj) skip |= (jj < j && taken[jj] == c);
        if (skip) continue;
        const float v = z[c];
        if constexpr (WANT_NAN) any |= (v != v);
        if (bi == kNone || better(v, c, bv, bi)) {
            bv = v;
            bi = c;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if constexpr (WANT_NAN) any |= __shfl_xor(any, off);
        if (oi != kNone && (bi == kNone || better(ov, oi, bv, bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if constexpr (WANT_NAN) *nan = any != 0;
    val = bv;
    return bi;
}

// the first M classes of one row in that order (every lane gets all of them); M <= K
template <int M>
__device__ __forceinline__ void row_top(const float *__restrict__ z, int K, int lane, int (&idx)[M], float (&val)[M]) {
#pragma unroll
    for (int j = 0; j < M; ++j) idx[j] = row_next(z, K, lane, idx, j, val[j]);
}

// the first class of one row; nan: the row holds a NaN
__device__ __forceinline__ int row_first(const float *__restrict__ z, int K, int lane, bool &nan) {
    const int none[1] = {kNone};
    float val;
    return row_next<1, true>(z, K, lane, none, 0, val, &nan);
}

}  // namespace ee
