// ee_eot.hip - expectation over transformation (EOT) for APGD on a randomised defence: the gradient of an iterate is the mean of the input
// gradients of E forwards, each under a draw of its own, and the loss its bookkeeping sees is the mean of their row losses.
//
// One launch after each draw's backward:
//     ee_apgd_eot_acc_f32   g_acc <- g | g_acc + g, the last draw also * (1/E);  loss_acc (double) <- loss | loss_acc + loss, the last
//                           draw also loss_mean <- loss_acc / E
// k (the draw) and E are host values: the E draws of an iteration sit inside one captured graph, so k is a constant of its node.
// Pure traffic, 12 B per element (8 B at k == 0: the accumulator is not read, so whatever it held - NaNs included - is gone).
// No thread reads a value that another thread of the launch writes: element i of g_acc and sample b of loss_acc / loss_mean belong to
// one thread each, and g / loss are only read.
#include "ee_common.hpp"

namespace {

using namespace ee;

struct AccOp {
    bool first, last;
    float inv;
    // the add is rounded before the multiply: two operations, never one fused one (the file is compiled with -ffp-contract=off)
    __device__ __forceinline__ float operator()(float acc, float g) const {
        const float s = first ? g : acc + g;
        return last ? s * inv : s;
    }
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void eot_acc_kernel(float *g_acc, const float *__restrict__ g, double *loss_acc,
                                                         const float *__restrict__ loss, float *__restrict__ loss_mean, int64_t n, int B,
                                                         int first, int last, float inv, double E) {
    const AccOp op{first != 0, last != 0, inv};
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int64_t b = i; b < B; b += stride) {  // the row losses: B values, the first threads of the grid
        const double s = first ? static_cast<double>(loss[b]) : loss_acc[b] + static_cast<double>(loss[b]);
        loss_acc[b] = s;
        if (last) loss_mean[b] = static_cast<float>(s / E);
    }
    if (VEC == 4) {  // 16-byte bases; a vector may straddle samples - the operation does not depend on the sample
        const int64_t nv = n >> 2;
        for (int64_t v = i; v < nv; v += stride) {
            const float4 vg = reinterpret_cast<const float4 *>(g)[v];
            float4 va = vg;
            if (!first) va = reinterpret_cast<const float4 *>(g_acc)[v];
            float4 r;
            r.x = op(va.x, vg.x);
            r.y = op(va.y, vg.y);
            r.z = op(va.z, vg.z);
            r.w = op(va.w, vg.w);
            reinterpret_cast<float4 *>(g_acc)[v] = r;
        }
        for (int64_t e = (nv << 2) + i; e < n; e += stride) g_acc[e] = op(first ? 0.0f : g_acc[e], g[e]);
    } else {
        for (int64_t e = i; e < n; e += stride) g_acc[e] = op(first ? 0.0f : g_acc[e], g[e]);
    }
}

}  // namespace

EE_API int ee_apgd_eot_acc_f32(float *g_acc, const float *g, double *loss_acc, const float *loss, float *loss_mean, int k, int E, int64_t B,
                               int64_t per_sample, void *stream) {
    if (E < 1 || k < 0 || k >= E) return EE_ERR_SHAPE;
    if (B < 0 || B > INT32_MAX || per_sample < 0 || (per_sample > 0 && B > INT64_MAX / per_sample)) return EE_ERR_SHAPE;
    const int64_t n = B * per_sample;
    if (n == 0) return EE_OK;  // an empty batch is no attack: nothing is launched
    if (!g_acc || !g || !loss_acc || !loss || !loss_mean) return EE_ERR_NULL;
    if (g_acc == g) return EE_ERR_SHAPE;  // the accumulator is written while other draws' gradients are read: never the same tensor
    if (!aligned4(g_acc) || !aligned4(g) || !aligned4(loss) || !aligned4(loss_mean) || (reinterpret_cast<uintptr_t>(loss_acc) & 7u) != 0)
        return EE_ERR_ALIGN;
    const bool vec = aligned16(g_acc) && aligned16(g);
    const int64_t work = vec ? (n + 3) / 4 : n;
    const unsigned blocks = grid_for(work > B ? work : B);
    const float inv = 1.0f / static_cast<float>(E);
    const int first = k == 0, last = k == E - 1;
    if (vec)
        EE_LAUNCH(eot_acc_kernel<4>, dim3(blocks), dim3(kBlock), 0, as_stream(stream), g_acc, g, loss_acc, loss, loss_mean, n,
                  static_cast<int>(B), first, last, inv, static_cast<double>(E));
    else
        EE_LAUNCH(eot_acc_kernel<1>, dim3(blocks), dim3(kBlock), 0, as_stream(stream), g_acc, g, loss_acc, loss, loss_mean, n,
                  static_cast<int>(B), first, last, inv, static_cast<double>(E));
    return launch_status();
}
