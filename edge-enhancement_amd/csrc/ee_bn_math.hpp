// ee_bn_math.hpp - the BatchNorm expressions, each written once.
//
// ee_bn.hip's kernel families and the convolution kernels that fold a BatchNorm in (ee_fuse.hpp) promise equal BITS: fused = unfused,
// dual = two calls, mask-from-x = mask-from-y, every workgroup the same statistics.  The build keeps expressions as written
// (-ffp-contract=off -fno-fast-math), so the promise holds exactly when every kernel evaluates the same expression tree - these.
// Operand order and parentheses here are part of the contract.
#pragma once
#include "ee_common.hpp"

namespace ee {

__device__ __forceinline__ float bn_invstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }
// invstd * gamma: the forward's slope and the backward's weight (one product)
__device__ __forceinline__ float bn_gain(float invstd, const float *gamma, int c) { return invstd * (gamma ? gamma[c] : 1.0f); }
__device__ __forceinline__ float bn_shift(const float *beta, int c) { return beta ? beta[c] : 0.0f; }

// ReLU that keeps NaN, as torch.relu does
__device__ __forceinline__ float relu_nan(float r) { return r > 0.0f ? r : (r != r ? r : 0.0f); }
__device__ __forceinline__ float4 relu_nan4(float4 r) { return make_float4(relu_nan(r.x), relu_nan(r.y), relu_nan(r.z), relu_nan(r.w)); }

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 scale4(float w, float4 v) { return make_float4(w * v.x, w * v.y, w * v.z, w * v.w); }
// threshold_backward: v where m > 0, else 0
__device__ __forceinline__ float mask1(float v, float m) { return m > 0.0f ? v : 0.0f; }
__device__ __forceinline__ float4 mask4(float4 v, float4 m) { return make_float4(mask1(v.x, m.x), mask1(v.y, m.y), mask1(v.z, m.z), mask1(v.w, m.w)); }

// forward: y = (v - mean) * a + b0, a = bn_gain
__device__ __forceinline__ float bn_affine(float v, float mean, float a, float b0) { return (v - mean) * a + b0; }
__device__ __forceinline__ float4 bn_affine4(float4 v, float mean, float a, float b0) {
    return make_float4(bn_affine(v.x, mean, a, b0), bn_affine(v.y, mean, a, b0), bn_affine(v.z, mean, a, b0), bn_affine(v.w, mean, a, b0));
}
__device__ __forceinline__ float bn_xhat(float v, float mean, float invstd) { return (v - mean) * invstd; }
__device__ __forceinline__ float4 bn_xhat4(float4 v, float mean, float invstd) {
    return make_float4(bn_xhat(v.x, mean, invstd), bn_xhat(v.y, mean, invstd), bn_xhat(v.z, mean, invstd), bn_xhat(v.w, mean, invstd));
}
// backward: dx = w * ((dz - m1) - xhat * m2), w = bn_gain, m1 / m2 = mean(dz) / mean(dz * xhat) in training mode and 0 in eval mode
__device__ __forceinline__ float bn_dx(float w, float g, float m1, float h, float m2) { return w * ((g - m1) - h * m2); }
__device__ __forceinline__ float4 bn_dx4(float w, float4 g, float m1, float4 h, float m2) {
    return make_float4(bn_dx(w, g.x, m1, h.x, m2), bn_dx(w, g.y, m1, h.y, m2), bn_dx(w, g.z, m1, h.z, m2), bn_dx(w, g.w, m1, h.w, m2));
}

// what a float4 adds to a lane's running sum: pairs first
__device__ __forceinline__ float quad_sum(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float quad_dot(float4 g, float4 h) { return (g.x * h.x + g.y * h.y) + (g.z * h.z + g.w * h.w); }
__device__ __forceinline__ float quad_sqdev(float4 v, float mean) {
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, d = v.w - mean;
    return (a * a + b * b) + (c * c + d * d);
}

// What a training-mode forward leaves behind for channel c (ONE lane calls it): the batch statistics for the backward pass and
// nn.BatchNorm2d's step of the running statistics (momentum, unbiased variance of the n values); running_mean null: no such step.
__device__ __forceinline__ void bn_commit_stats(int c, float mean, float var, float invstd, float n, float momentum, float *save_mean, float *save_invstd,
                                                float *running_mean, float *running_var) {
    save_mean[c] = mean;
    save_invstd[c] = invstd;
    if (running_mean) {
        const float unbiased = (n > 1.0f) ? var * (n / (n - 1.0f)) : var;
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * unbiased;
    }
}

// statistics that already exist: those the training-mode forward saved, or the running ones (eval mode, either direction)
struct BnStats {
    float mean, invstd;
};
__device__ __forceinline__ BnStats bn_known_stats(int training, const float *save_mean, const float *save_invstd, const float *running_mean,
                                                  const float *running_var, float eps, int c) {
    return BnStats{training ? save_mean[c] : running_mean[c], training ? save_invstd[c] : bn_invstd(running_var[c], eps)};
}

// The ReLU mask of the backward is y > 0.  Without a residual branch y = relu((x - mean) * a + b0), so the mask can be recomputed
// from x - which the backward reads anyway - with bn_affine (the forward's bits) instead of reading y: one tensor less.  `on` selects it.
struct MaskArgs {
    int on;
    float a, b0;  // bn_gain, beta
};
__device__ __forceinline__ MaskArgs mask_args(const float *y, const float *gamma, const float *beta, float invstd, int c) {
    MaskArgs m;
    m.on = y == nullptr;
    m.a = bn_gain(invstd, gamma, c);
    m.b0 = (beta && m.on) ? beta[c] : 0.0f;
    return m;
}

}  // namespace ee
