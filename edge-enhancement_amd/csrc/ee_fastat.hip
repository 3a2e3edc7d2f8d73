// ee_fastat.hip - the three element-wise launches of fast adversarial training (FGSM from a random start; ImageNet/fgsm_imagenet/
// main_fast.py:224-266 and lib/validation.py:51-57), gfx950.  The contracts - expressions, ties, NaN, aliasing, error codes - are in
// include/eeadv.h; DESIGN.md section 28 has the step they serve.
//
// All three are HBM-bound streams: every lane moves 16 B per access where the sizes and addresses allow it and a word otherwise (the
// same bits either way), the grid is capped at 8 workgroups of 256 threads per CU and grid-strides the rest (ee_common.hpp grid_for).
// The arithmetic is that of ee_elementwise.hip's InitOp / FreeAtMaskedOp / init_rng_kernel<0>, operation for operation.
#include <math.h>

#include "ee_common.hpp"

namespace {

using namespace ee;

// ---- start: delta = noise or a fresh U(-eps, eps) draw, in1 = clamp(x + delta, 0, 1) -------------------------------------------------
// One thread per group of four elements - the unit of one Philox call.  VEC = 4: n % 4 == 0 and every pointer 16-byte aligned.
template <int VEC, bool DRAW>
__global__ __launch_bounds__(kBlock) void fastat_start_kernel(float *delta, float *__restrict__ in1, const float *__restrict__ x,
                                                              const float *noise, int64_t n, float eps, uint64_t seed,
                                                              const uint64_t *__restrict__ step) {
    const Philox rng(seed);
    const uint64_t offset = DRAW ? (step[0] << 32) : 0;
    const float span = eps - (-eps);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t nv = (n + 3) >> 2;
    for (int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; v < nv; v += stride) {
        const int64_t base = v << 2;
        float d[4], xv[4];
        if (DRAW) {
            const uint4 r = rng(offset + static_cast<uint64_t>(v));
            const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)  // ee_pgd_init_rng_f32 with x0 = 0, lo = -eps, hi = eps
                d[k] = tclamp(0.0f + (u01(w[k]) * span + (-eps)), -eps, eps);
        } else if (VEC == 4) {
            const float4 t = reinterpret_cast<const float4 *>(noise)[v];
            d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = base + k < n ? noise[base + k] : 0.0f;
        }
        if (VEC == 4) {
            const float4 t = reinterpret_cast<const float4 *>(x)[v];
            xv[0] = t.x, xv[1] = t.y, xv[2] = t.z, xv[3] = t.w;
            reinterpret_cast<float4 *>(delta)[v] = make_float4(d[0], d[1], d[2], d[3]);
            reinterpret_cast<float4 *>(in1)[v] = make_float4(tclamp(xv[0] + d[0], 0.0f, 1.0f), tclamp(xv[1] + d[1], 0.0f, 1.0f),
                                                             tclamp(xv[2] + d[2], 0.0f, 1.0f), tclamp(xv[3] + d[3], 0.0f, 1.0f));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (base + k < n) {
                    delta[base + k] = d[k];
                    in1[base + k] = tclamp(x[base + k] + d[k], 0.0f, 1.0f);
                }
        }
    }
}

// ---- ascend: the masked free-AT noise update and the descend pass's input in one sweep; then the step counter -------------------------
struct AscendOp {
    float alpha, eps;
    __device__ __forceinline__ void operator()(float d, float g, float x, float &d_new, float &in) const {
        const float s = x + d;  // main_fast.py:234-235: in1 = (x + delta).clamp_(0, 1); the clamp passes the gradient on [0, 1]
        const float gd = (s >= 0.0f && s <= 1.0f) ? g : 0.0f;
        d_new = tclamp(d + alpha * sgn(gd), -eps, eps);  // :246-248
        in = tclamp(x + d_new, 0.0f, 1.0f);              // :252-253
    }
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void fastat_ascend_kernel(float *delta, float *in1, const float *g, const float *__restrict__ x,
                                                               int64_t n, AscendOp op, uint64_t *step) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (VEC == 4) {
        for (int64_t v = i; v < (n >> 2); v += stride) {
            const float4 vd = reinterpret_cast<const float4 *>(delta)[v];
            const float4 vg = reinterpret_cast<const float4 *>(g)[v];
            const float4 vx = reinterpret_cast<const float4 *>(x)[v];
            float4 rd, ri;
            op(vd.x, vg.x, vx.x, rd.x, ri.x);
            op(vd.y, vg.y, vx.y, rd.y, ri.y);
            op(vd.z, vg.z, vx.z, rd.z, ri.z);
            op(vd.w, vg.w, vx.w, rd.w, ri.w);
            reinterpret_cast<float4 *>(delta)[v] = rd;
            reinterpret_cast<float4 *>(in1)[v] = ri;
        }
    } else {
        for (int64_t k = i; k < n; k += stride) {
            float rd, ri;
            op(delta[k], g[k], x[k], rd, ri);
            delta[k] = rd;
            in1[k] = ri;
        }
    }
    // nothing in this launch reads the counter: ee_fastat_start_f32 of the NEXT step does, a launch later on the same stream
    if (step && i == 0) step[0] = step[0] + 1;
}

// ---- keep: final[b] = x[b] where the model is fooled (or everywhere, first restart) --------------------------------------------------
// torch.max(1)[1]: a NaN beats every number, the first NaN / the first of equal maxima wins
struct Best {
    float v;
    int k;
};
__device__ __forceinline__ bool beats(const Best &a, const Best &b) {
    const bool na = a.v != a.v, nb = b.v != b.v;
    if (na != nb) return na;
    if (!na && a.v != b.v) return a.v > b.v;
    return a.k < b.k;
}

// workgroup id = row * chunks + chunk.  Every workgroup of a row finds the row's arg-max for itself (K floats, read once from HBM and
// `chunks - 1` times from L2) and copies its chunk of the row, so there is one launch and no flag array between two.
template <int VEC>
__global__ __launch_bounds__(kBlock) void fastat_keep_kernel(float *__restrict__ final_, const float *__restrict__ x,
                                                             const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                             int K, int64_t per, int chunks, int first) {
    __shared__ Best sh[kBlock / kWave];
    const int64_t b = blockIdx.x / chunks;
    const int chunk = static_cast<int>(blockIdx.x - b * chunks);
    if (!first) {
        const float *row = logits + b * K;
        Best best{-INFINITY, 0x7fffffff};
        for (int k = threadIdx.x; k < K; k += kBlock) {
            const Best c{row[k], k};
            if (beats(c, best)) best = c;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const Best c{__shfl_down(best.v, o, kWave), __shfl_down(best.k, o, kWave)};
            if (beats(c, best)) best = c;
        }
        if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = best;
        __syncthreads();
        best = sh[0];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w)
            if (beats(sh[w], best)) best = sh[w];
        if (static_cast<int64_t>(best.k) == labels[b]) return;  // still classified correctly: the row keeps what it holds (uniform per workgroup)
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(x) + b * per;
    uint32_t *dst = reinterpret_cast<uint32_t *>(final_) + b * per;
    const int64_t stride = static_cast<int64_t>(chunks) * kBlock;
    const int64_t i = static_cast<int64_t>(chunk) * kBlock + threadIdx.x;
    if (VEC == 4) {
        for (int64_t v = i; v < (per >> 2); v += stride) reinterpret_cast<uint4 *>(dst)[v] = reinterpret_cast<const uint4 *>(src)[v];
    } else {
        for (int64_t k = i; k < per; k += stride) dst[k] = src[k];
    }
}

}  // namespace

EE_API int ee_fastat_start_f32(float *delta, float *in1, const float *x, const float *noise, int64_t n, float eps, uint64_t seed,
                               const uint64_t *step, void *stream) {
    // n / 4 < 2^32 leaves at most 2^32 groups of four, the partial last one included: group indices 0 .. 2^32 - 1 stay in the counter's low word
    if (n < 0 || (n >> 2) >= (int64_t(1) << 32) || !(eps >= 0.0f)) return EE_ERR_SHAPE;
    if (n == 0) return EE_OK;
    if (!delta || !in1 || !x || (!noise && !step)) return EE_ERR_NULL;
    if (!aligned4(delta) || !aligned4(in1) || !aligned4(x) || (noise && !aligned4(noise)) ||
        (!noise && (reinterpret_cast<uintptr_t>(step) & 7u)))
        return EE_ERR_ALIGN;
    const bool vec = (n & 3) == 0 && aligned16(delta) && aligned16(in1) && aligned16(x) && (!noise || aligned16(noise));
    const unsigned grid = grid_for((n + 3) / 4);
    hipStream_t s = as_stream(stream);
    if (noise) {
        if (vec)
            EE_LAUNCH((fastat_start_kernel<4, false>), dim3(grid), dim3(kBlock), 0, s, delta, in1, x, noise, n, eps, seed, step);
        else
            EE_LAUNCH((fastat_start_kernel<1, false>), dim3(grid), dim3(kBlock), 0, s, delta, in1, x, noise, n, eps, seed, step);
    } else {
        if (vec)
            EE_LAUNCH((fastat_start_kernel<4, true>), dim3(grid), dim3(kBlock), 0, s, delta, in1, x, noise, n, eps, seed, step);
        else
            EE_LAUNCH((fastat_start_kernel<1, true>), dim3(grid), dim3(kBlock), 0, s, delta, in1, x, noise, n, eps, seed, step);
    }
    return launch_status();
}

EE_API int ee_fastat_ascend_f32(float *delta, float *in1, const float *g, const float *x, int64_t n, float alpha, float eps,
                                uint64_t *step, void *stream) {
    if (n < 0) return EE_ERR_SHAPE;
    if (n == 0) return EE_OK;  // no launch: the counter does not move either
    if (!delta || !in1 || !g || !x) return EE_ERR_NULL;
    if (!aligned4(delta) || !aligned4(in1) || !aligned4(g) || !aligned4(x) || (reinterpret_cast<uintptr_t>(step) & 7u)) return EE_ERR_ALIGN;
    const bool vec = (n & 3) == 0 && aligned16(delta) && aligned16(in1) && aligned16(g) && aligned16(x);
    const AscendOp op{alpha, eps};
    if (vec)
        EE_LAUNCH(fastat_ascend_kernel<4>, dim3(grid_for(n / 4)), dim3(kBlock), 0, as_stream(stream), delta, in1, g, x, n, op, step);
    else
        EE_LAUNCH(fastat_ascend_kernel<1>, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), delta, in1, g, x, n, op, step);
    return launch_status();
}

EE_API int ee_fastat_keep_f32(float *final_, const float *x, const float *logits, const int64_t *labels, int64_t B, int64_t K,
                              int64_t per_sample, int first, void *stream) {
    if (B < 0 || B > 0x7fffffff || per_sample < 1 || (!first && (K < 1 || K > 0x7fffffff))) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!final_ || !x || (!first && (!logits || !labels))) return EE_ERR_NULL;
    if (final_ == x) return EE_ERR_SHAPE;
    if (!aligned4(final_) || !aligned4(x) || (!first && (!aligned4(logits) || (reinterpret_cast<uintptr_t>(labels) & 7u)))) return EE_ERR_ALIGN;
    const bool vec = (per_sample & 3) == 0 && aligned16(final_) && aligned16(x);
    // a workgroup moves 4 accesses per lane before it strides; the grid stays within the streaming cap once B itself is below it
    const int64_t units = vec ? per_sample >> 2 : per_sample;
    int64_t chunks = (units + 4 * kBlock - 1) / (4 * kBlock);
    const int64_t cap = kMaxGrid / B > 1 ? kMaxGrid / B : 1;
    chunks = chunks > cap ? cap : chunks;
    const unsigned grid = static_cast<unsigned>(B * chunks);
    if (vec)
        EE_LAUNCH(fastat_keep_kernel<4>, dim3(grid), dim3(kBlock), 0, as_stream(stream), final_, x, logits, labels, static_cast<int>(K),
                  per_sample, static_cast<int>(chunks), first);
    else
        EE_LAUNCH(fastat_keep_kernel<1>, dim3(grid), dim3(kBlock), 0, as_stream(stream), final_, x, logits, labels, static_cast<int>(K),
                  per_sample, static_cast<int>(chunks), first);
    return launch_status();
}
