// ee_sqatk.hip - the Square attack (Andriushchenko et al. 2020, Linf, the schedule of AutoAttack's "standard" version) around the classifier.
// The ATTACK, not the Add_Square defence of ee_square.hip.  One query is two launches around an eval-mode forward:
//     ee_sqatk_step_f32    commit the accepted proposal (x_best <- x_new where flags[b]), then write the next proposal into x_new
//     ee_sqatk_margin_f32  logits -> margin z_y - max_{j != y} z_j, accept / reject per sample, counter += 1   (one wavefront per row)
// and ee_sqatk_init_f32 writes the striped start once per attack.  The window of proposal i and sample b and the stripes of the start come
// from Philox4x32-10 at counters that depend on (i, b) / (b, c, w >> 7) only: no sequential random state, and nothing a host value
// changes from query to query, so one captured graph serves every query.  No launch writes a scalar another thread of the same launch
// reads: step only reads flags, margin_min and the counter; margin owns row b's scalars in row b's wavefront and never reads the counter
// it advances.
#include <math.h>

#include "ee_rows.hpp"
#include "ee_sqatk.hpp"

namespace {

using namespace ee;

// ---- start ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void init_kernel(float *__restrict__ x_best, float *__restrict__ x_new, const float *__restrict__ x0,
                                                      const int64_t *__restrict__ seed, int64_t n, int C, int H, int W, float eps) {
    const Philox ph(static_cast<uint64_t>(seed[0]));
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t HW = static_cast<int64_t>(H) * W;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int64_t plane = e / HW;  // b * C + c
        const int w = static_cast<int>((e - plane * HW) % W);
        const uint4 r = ph((static_cast<uint64_t>(plane) << 32) | static_cast<uint32_t>(w >> 7), kStreamStripe);
        const int k = (w >> 5) & 3;
        const uint32_t word = k == 0 ? r.x : (k == 1 ? r.y : (k == 2 ? r.z : r.w));
        const float v = tclamp(x0[e] + (((word >> (w & 31)) & 1u) ? eps : -eps), 0.0f, 1.0f);
        x_best[e] = v;
        x_new[e] = v;
    }
}

// ---- margin and the accept decision --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void margin_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels, int B, int K,
                                                        float *__restrict__ margin_out, float *margin_min, int *queries, int *__restrict__ flags,
                                                        int *counter) {
    const int lane = threadIdx.x & (kWave - 1);
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row == 0 && lane == 0) counter[0] = counter[0] + 1;  // nobody reads the counter in this launch
    if (row >= B) return;
    const float *z = logits + static_cast<size_t>(row) * K;
    const int64_t y = labels[row];
    float other = -INFINITY;
    int nan = (y < 0 || y >= K) ? 1 : 0;  // a label outside the row is never dereferenced
    for (int k = lane; k < K; k += kWave) {
        const float v = z[k];
        nan |= (v != v);
        if (k != y) other = fmaxf(other, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        other = fmaxf(other, __shfl_xor(other, off));
        nan |= __shfl_xor(nan, off);
    }
    if (lane != 0) return;
    const float m = nan ? NAN : z[y] - other;  // one fp32 difference of two inputs; inf - inf is NaN by itself
    margin_out[row] = m;
    const float best = margin_min[row];
    int accept = 0;
    if (!(best <= 0.0f)) {  // not fooled: this forward was a query of the sample
        queries[row] = queries[row] + 1;
        if (m < best) {  // false for a NaN margin
            margin_min[row] = m;
            accept = 1;
        }
    }
    flags[row] = accept;
}

// ---- commit and proposal -------------------------------------------------------------------------------------------------------------
struct Sample {
    bool commit, propose;
    int vh, vw;
    uint32_t bits;
};

__device__ __forceinline__ Sample sample_of(int64_t b, const int *__restrict__ flags, const float *__restrict__ margin_min, const Philox &ph, int it, int s,
                                            int H, int W) {
    Sample r;
    r.commit = flags[b] != 0;
    r.propose = s > 0 && !(margin_min[b] <= 0.0f);
    r.vh = r.vw = 0;
    r.bits = 0u;
    if (r.propose) {
        const WindowDraw d = draw_window(ph, it, b, s, H, W, kStreamWindow);
        r.vh = d.vh;
        r.vw = d.vw;
        r.bits = d.z;
    }
    return r;
}

__device__ __forceinline__ float propose(float xb, float x0, const Sample &sm, int c, int h, int w, int s, float eps) {
    const bool in = h >= sm.vh && h < sm.vh + s && w >= sm.vw && w < sm.vw + s;
    const float delta = in ? (((sm.bits >> c) & 1u) ? 2.0f * eps : -2.0f * eps) : 0.0f;
    return proj_linf(xb + delta, x0, eps);
}

// what a step launch knows apart from the element it is at
struct Step {
    float *x_best, *x_new;
    const float *x0;
    const int *flags;
    const float *margin_min;
    Philox ph;
    int it, s, H, W, HW;
    int64_t per_sample;
    float eps;
};

// one element's turn: its sample's decision, the commit, the proposal
__device__ __forceinline__ void element_turn(const Step &k, int64_t e) {
    const int64_t b = e / k.per_sample;
    const int r = static_cast<int>(e - b * k.per_sample);
    const Sample sm = sample_of(b, k.flags, k.margin_min, k.ph, k.it, k.s, k.H, k.W);
    if (!sm.commit && !sm.propose) return;
    float xb;
    if (sm.commit) {
        xb = k.x_new[e];
        k.x_best[e] = xb;
    } else {
        xb = k.x_best[e];
    }
    if (!sm.propose) return;
    const int c = r / k.HW, h = (r - c * k.HW) / k.W, w = r - c * k.HW - h * k.W;
    k.x_new[e] = propose(xb, k.x0[e], sm, c, h, w, k.s, k.eps);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void step_kernel(float *x_best, float *x_new, const float *__restrict__ x0, const int *__restrict__ flags,
                                                      const float *__restrict__ margin_min, const int *__restrict__ counter,
                                                      const int *__restrict__ sizes, int n_sizes, const int64_t *__restrict__ seed, int64_t n,
                                                      int C, int H, int W, float eps) {
    const int it = counter[0];
    int s = (it >= 0 && it < n_sizes) ? sizes[it] : 0;  // 0: no proposal in this launch (commit only)
    if (s < 1 || s > H || s > W) s = 0;                 // a size the window arithmetic cannot take is no proposal either
    const int HW = H * W;
    const int64_t per_sample = static_cast<int64_t>(C) * HW;
    const Step k{x_best, x_new, x0, flags, margin_min, Philox(static_cast<uint64_t>(seed[0])), it, s, H, W, HW, per_sample, eps};
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t nv = VEC == 4 ? (n >> 2) : 0;
    for (int64_t v = i; v < nv; v += stride) {
        const int64_t base = v << 2;
        const int64_t b = base / per_sample;
        const int r = static_cast<int>(base - b * per_sample);
        if (r + 4 > per_sample) {  // a vector across two (or more) samples: element by element
            for (int j = 0; j < 4; ++j) element_turn(k, base + j);
            continue;
        }
        // the four elements belong to one sample (they may straddle rows and channels): element_turn's lines on float4 accesses
        const Sample sm = sample_of(b, flags, margin_min, k.ph, it, s, H, W);
        if (!sm.commit && !sm.propose) continue;
        float4 xb;
        if (sm.commit) {
            xb = reinterpret_cast<const float4 *>(x_new)[v];
            reinterpret_cast<float4 *>(x_best)[v] = xb;
        } else {
            xb = reinterpret_cast<const float4 *>(x_best)[v];
        }
        if (!sm.propose) continue;
        const float4 v0 = reinterpret_cast<const float4 *>(x0)[v];
        int c = r / HW, h = (r - c * HW) / W, w = r - c * HW - h * W;
        const float in[4] = {xb.x, xb.y, xb.z, xb.w}, o0[4] = {v0.x, v0.y, v0.z, v0.w};
        float out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[j] = propose(in[j], o0[j], sm, c, h, w, s, eps);
            if (++w == W) {
                w = 0;
                if (++h == H) h = 0, ++c;
            }
        }
        reinterpret_cast<float4 *>(x_new)[v] = make_float4(out[0], out[1], out[2], out[3]);
    }
    for (int64_t e = (nv << 2) + i; e < n; e += stride) element_turn(k, e);
}

}  // namespace

EE_API int ee_sqatk_init_f32(float *x_best, float *x_new, const float *x0, const int64_t *seed, int B, int C, int H, int W, float eps,
                             void *stream) {
    int rc = sqatk_check_shape(B, C, H, W);
    if (rc != EE_OK) return rc;
    if (B == 0) return EE_OK;
    if ((rc = sqatk_check_ptrs(seed, {x_best, x_new, x0})) != EE_OK) return rc;
    const int64_t n = static_cast<int64_t>(B) * C * H * W;
    ProfScope prof(EE_K_SQATK_INIT, as_stream(stream));
    EE_LAUNCH(init_kernel, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), x_best, x_new, x0, seed, n, C, H, W, eps);
    return launch_status();
}

EE_API int ee_sqatk_margin_f32(const float *logits, const int64_t *labels, int B, int K, float *margin_out, float *margin_min, int *queries,
                               int *flags, int *counter, void *stream) {
    if (B < 0 || K < 2 || K > 65536) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;  // an empty batch is no query: nothing is launched, the counter stays
    if (!logits || !labels || !margin_out || !margin_min || !queries || !flags || !counter) return EE_ERR_NULL;
    if (!aligned4(logits) || !aligned4(margin_out) || !aligned4(margin_min) || !aligned4(queries) || !aligned4(flags) || !aligned4(counter) ||
        (reinterpret_cast<uintptr_t>(labels) & 7u))
        return EE_ERR_ALIGN;
    ProfScope prof(EE_K_SQATK_MARGIN, as_stream(stream));
    EE_LAUNCH(margin_kernel, dim3(row_grid(B)), dim3(kBlock), 0, as_stream(stream), logits,
              labels, B, K, margin_out, margin_min, queries, flags, counter);
    return launch_status();
}

EE_API int ee_sqatk_step_f32(float *x_best, float *x_new, const float *x0, const int *flags, const float *margin_min, const int *counter,
                             const int *sizes, int n_sizes, const int64_t *seed, int B, int C, int H, int W, float eps, void *stream) {
    int rc = sqatk_check_shape(B, C, H, W);
    if (rc != EE_OK) return rc;
    if (n_sizes < 0) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if ((rc = sqatk_check_ptrs(seed, {x_best, x_new, x0, flags, margin_min, counter}, n_sizes > 0, {sizes})) != EE_OK) return rc;
    const int64_t n = static_cast<int64_t>(B) * C * H * W;
    const bool vec = aligned16(x_best) && aligned16(x_new) && aligned16(x0);
    ProfScope prof(EE_K_SQATK_STEP, as_stream(stream));
    if (vec)
        EE_LAUNCH(step_kernel<4>, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, as_stream(stream), x_best, x_new, x0, flags, margin_min, counter,
                  sizes, n_sizes, seed, n, C, H, W, eps);
    else
        EE_LAUNCH(step_kernel<1>, dim3(grid_for(n)), dim3(kBlock), 0, as_stream(stream), x_best, x_new, x0, flags, margin_min, counter, sizes,
                  n_sizes, seed, n, C, H, W, eps);
    return launch_status();
}
