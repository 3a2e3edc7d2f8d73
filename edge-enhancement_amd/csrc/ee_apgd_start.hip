// ee_apgd_start.hip - APGD restarts: the two launches a restart adds around the captured iterations, both outside
// the graph.
//     ee_apgd_start_f32   x <- the start point of restart r >= 1, drawn on the device (or taken from injected noise) around x0
//     ee_apgd_merge_f32   the union across restarts: a sample some restart fooled keeps the point of the FIRST restart that fooled it
// One workgroup of 512 threads per sample in both (ee_sample.hpp).  Neither reads a host value that changes inside an attack, allocates or
// synchronises; a workgroup reads and writes the scalars of its own sample only.
#include <math.h>

#include "ee_sample.hpp"

namespace {

using namespace ee;

enum Metric : int { kLinf = 0, kL2 = 1, kL1 = 2 };  // EE_FAB_METRIC_*: the threat model of the run

// ---- the start of a restart ---------------------------------------------------------------------------------------------------------------
// The distribution of the project's restart 0 in each threat model, every operation rounded once in the order written:
//   kLinf  x = clamp(x0 + eps * t, 0, 1),        t = 2 u01 - 1                                    (one pass: no norm)
//   kL2    n = (float) sqrt(sum t_i^2) - the sum in double in the one order of ee_sample.hpp -, s = eps / (n + 1e-12f),
//          x = clamp(x0 + t * s, 0, 1),          t standard normal;   n not finite: the row is x0
//   kL1    x = x0 + t, unclamped,                t standard normal    (one pass; the run's own projection follows)
// DRAW: t comes from start_draw4 under kStreamApgdStart, else from the row of `noise`.  RES (kL2 only has two passes) keeps t in registers
// between the norm pass and the write pass; the streaming path reads or draws it again.
template <bool RES, bool VEC, int M, bool DRAW>
__global__ __launch_bounds__(kSampleBlock) void start_kernel(float *__restrict__ x, const float *__restrict__ x0, const float *__restrict__ noise,
                                                             int64_t D, float eps, uint64_t seed) {
    const int b = blockIdx.x;
    const int64_t off = static_cast<int64_t>(b) * D;
    const float *x0r = x0 + off, *nr = DRAW ? nullptr : noise + off;
    float *xr = x + off;
    const Philox ph(seed);
    const int groups = groups_of(D);

    float keep[kSampleElems];
    float s = eps;
    bool live = true;  // uniform over the workgroup
    if constexpr (M == kL2) {
        // pass 1: the norm of the draw; the resident path keeps the draw in keep[]
        __shared__ double sh[2 * kSampleWaves];
        SampleReducer red{sh};
        double acc = 0.0;
        auto first = [&](int g) {
            float t[4];
            start_draw4<kStreamApgdStart, false, DRAW, VEC>(ph, nr, b, group_element(g), D, t);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = fma(static_cast<double>(t[j]), static_cast<double>(t[j]), acc);  // the square of a float is exact in double
                if (RES) keep[g * 4 + j] = t[j];
            }
        };
        if (RES) {
#pragma unroll
            for (int g = 0; g < kSampleVecs; ++g) first(g);
        } else {
            for (int g = 0; g < groups; ++g) first(g);
        }
        const float n = static_cast<float>(sqrt(red.sum(acc)));
        live = isfinite(n);
        s = eps / (n + 1e-12f);
    }

    // the write pass (the only one of kLinf and kL1)
    auto second = [&](int g) {
        const int64_t e = group_element(g);
        float t[4], ov[4], out[4];
        if (RES && M == kL2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = keep[g * 4 + j];
        } else {
            start_draw4<kStreamApgdStart, M == kLinf, DRAW, VEC>(ph, nr, b, e, D, t);
        }
        load4<VEC>(x0r, e, D, ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (M == kLinf)
                out[j] = tclamp(ov[j] + eps * t[j], 0.0f, 1.0f);
            else if constexpr (M == kL2)
                out[j] = live ? tclamp(ov[j] + t[j] * s, 0.0f, 1.0f) : ov[j];
            else
                out[j] = ov[j] + t[j];
        }
        store4<VEC>(xr, e, D, out);
    };
    if (RES) {
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) second(g);
    } else {
        for (int g = 0; g < groups; ++g) second(g);
    }
}

// ---- the union across restarts --------------------------------------------------------------------------------------------------------------
// Sample b, with robust_* int flags (!= 0: still correctly classified) and the best row losses:
//   first:  robust_all = robust_run, loss_all = loss_run, adv_all[b] = x_best_adv[b] if robust_run == 0
//   else:   robust_all != 0 && robust_run == 0 -> adv_all[b] = x_best_adv[b], robust_all = 0;   loss_all = loss_run > loss_all ? loss_run : loss_all
// A row that is fooled already is never written again: the first fooling point stays.  Every thread reads the two flags before the barrier,
// thread 0 writes them after it.  Rows are copied as bits, 16 bytes at a time where both row starts are 16-byte aligned (decided per row,
// as ee_cascade.hip does: with per_sample % 4 != 0 every other row is not), word by word otherwise.
__global__ __launch_bounds__(kSampleBlock) void merge_kernel(uint32_t *__restrict__ adv_all, int *robust_all, float *loss_all,
                                                             const uint32_t *__restrict__ x_best_adv, const int *__restrict__ robust_run,
                                                             const float *__restrict__ loss_run, int64_t D, int first) {
    const int b = blockIdx.x;
    const int rr = robust_run[b];
    const int ra = first ? 1 : robust_all[b];
    const bool copy = ra != 0 && rr == 0;  // uniform over the workgroup
    __syncthreads();
    if (threadIdx.x == 0) {
        const float lr = loss_run[b];
        if (first) {
            robust_all[b] = rr;
            loss_all[b] = lr;
        } else {
            if (copy) robust_all[b] = 0;
            const float la = loss_all[b];
            loss_all[b] = lr > la ? lr : la;
        }
    }
    if (!copy) return;
    const uint32_t *src = x_best_adv + static_cast<int64_t>(b) * D;
    uint32_t *dst = adv_all + static_cast<int64_t>(b) * D;
    const int64_t t0 = threadIdx.x, stride = kSampleBlock;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        const int64_t D4 = D / 4;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int64_t i = t0; i < D4; i += stride) d4[i] = s4[i];
        for (int64_t i = 4 * D4 + t0; i < D; i += stride) dst[i] = src[i];  // the D % 4 words of the tail
    } else {
        for (int64_t i = t0; i < D; i += stride) dst[i] = src[i];
    }
}

bool bad_shape(int64_t B, int64_t per_sample) {
    return B < 0 || per_sample < 1 || B > INT32_MAX / 2 || per_sample > INT32_MAX || B > INT64_MAX / per_sample;
}

template <int M>
int launch_start(float *x, const float *x0, const float *noise, int64_t B, int64_t per_sample, float eps, uint64_t seed, bool resident,
                 void *stream) {
    const dim3 grid(static_cast<unsigned>(B)), block(kSampleBlock);
    sample_launch(resident, sample_vec(per_sample, x, x0, noise), [&](auto RES, auto VEC) {  // a null noise counts as aligned: it is not read
        if (noise)
            EE_LAUNCH((start_kernel<RES, VEC, M, false>), grid, block, 0, as_stream(stream), x, x0, noise, per_sample, eps, seed);
        else
            EE_LAUNCH((start_kernel<RES, VEC, M, true>), grid, block, 0, as_stream(stream), x, x0, noise, per_sample, eps, seed);
    });
    return launch_status();
}

}  // namespace

EE_API int ee_apgd_start_f32(float *x, const float *x0, const float *noise, int64_t B, int64_t per_sample, float eps, int metric, uint64_t seed,
                             int path, void *stream) {
    if (bad_shape(B, per_sample) || metric < kLinf || metric > kL1 || !(eps >= 0.0f)) return EE_ERR_SHAPE;
    bool resident;
    if (const int rc = sample_path(path, per_sample, &resident)) return rc;
    if (B == 0) return EE_OK;
    if (!x || !x0) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(x0) || !aligned4(noise)) return EE_ERR_ALIGN;
    ProfScope prof(EE_K_PGD_STEP, as_stream(stream));
    if (metric == kL2) return launch_start<kL2>(x, x0, noise, B, per_sample, eps, seed, resident, stream);
    if (metric == kL1) return launch_start<kL1>(x, x0, noise, B, per_sample, eps, seed, resident, stream);
    return launch_start<kLinf>(x, x0, noise, B, per_sample, eps, seed, resident, stream);
}

EE_API int ee_apgd_merge_f32(float *adv_all, int *robust_all, float *loss_all, const float *x_best_adv, const int *robust_run,
                             const float *loss_best_run, int64_t B, int64_t per_sample, int first, void *stream) {
    if (bad_shape(B, per_sample)) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!adv_all || !robust_all || !loss_all || !x_best_adv || !robust_run || !loss_best_run) return EE_ERR_NULL;
    if (!aligned4(adv_all) || !aligned4(robust_all) || !aligned4(loss_all) || !aligned4(x_best_adv) || !aligned4(robust_run) ||
        !aligned4(loss_best_run))
        return EE_ERR_ALIGN;
    ProfScope prof(EE_K_PGD_STEP, as_stream(stream));
    EE_LAUNCH(merge_kernel, dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), reinterpret_cast<uint32_t *>(adv_all),
              robust_all, loss_all, reinterpret_cast<const uint32_t *>(x_best_adv), robust_run, loss_best_run, per_sample, first != 0 ? 1 : 0);
    return launch_status();
}
