// ee_apgd_l2.hip - the step of APGD in the L2 threat model (Croce & Hein 2020, the L2 branch of APGD): the launch that stands in the place of
// ee_apgd_step_f32 in an L2 run.  Losses, bookkeeping, the copies and EOT do not know the norm (ee_apgd.hip, ee_eot.hip).
//
// Per sample, with a = 1 when counter[0] == 0, else 0.75, and tiny = 1e-12f - every operation rounded once in f32:
//     ng = ||g||_2                 sg = step / (ng + tiny)
//     z  = x + g * sg                                        (z = x when ng is not finite: no gradient step)
//     d  = z - x0      n1 = ||d||_2      s1 = min(eps, n1) / (n1 + tiny)
//     z  = clamp(x0 + d * s1, 0, 1)
//     m  = (x + (z - x) * a) + (x - xo) * (1 - a)
//     d  = m - x0      n2 = ||d||_2      s2 = min(eps, n2) / (n2 + tiny)
//     x_new = clamp(x0 + d * s2, 0, 1);   xo_new = x
// The rescale followed by the clamp is what is published; it is not the exact projection onto ball and box together.
//
// One workgroup per sample: the three norms depend on each other (n1 needs ng, n2 needs n1) and never cross a workgroup, so no launch writes
// a per-sample scalar that another workgroup of the same launch reads.  A norm is (float) sqrt(S), S the sum of the squares in double (the
// square of a float is exact there) in the one order of ee_sample.hpp, which the resident path (a sample's x, xo, g, x0 stay in registers
// across the three reductions) and the streaming path (every pass re-reads its inputs and recomputes z / m from the scalars already known)
// share, so the two return the same bits.  Every loop has a trip count fixed by per_sample.
// x and x_old are written in the final pass only, each element by the thread that read it.
#include <math.h>

#include "ee_sample.hpp"

namespace {

using namespace ee;

constexpr float kTiny = 1e-12f;

// the element-wise lines of the step; the scalars are filled in as the norms become known
struct L2Op {
    float a, b, eps;  // b = 1 - a
    bool take;        // ng is finite: the gradient step is taken
    float sg, s1, s2;
    __device__ __forceinline__ float d1(float x, float g, float x0) const {
        const float z = take ? x + g * sg : x;
        return z - x0;
    }
    __device__ __forceinline__ float d2(float x, float xo, float g, float x0) const {
        const float z = tclamp(x0 + d1(x, g, x0) * s1, 0.0f, 1.0f);
        const float m = (x + (z - x) * a) + (x - xo) * b;
        return m - x0;
    }
    __device__ __forceinline__ float next(float x, float xo, float g, float x0) const {
        return tclamp(x0 + d2(x, xo, g, x0) * s2, 0.0f, 1.0f);
    }
};

// min(eps, n) / (n + tiny), NaN in n propagating as torch.min does
__device__ __forceinline__ float rescale(float eps, float n) { return tmin(eps, n) / (n + kTiny); }

// RES: groups 0 .. kSampleVecs-1 of this thread live in rx / ro / rg / rc (zeros past D); otherwise every pass re-reads the four rows.
// The body sees (element, x, xo, g, x0) of every float4 group of the thread in the same order on both paths.
template <bool RES, bool VEC, class F>
__device__ __forceinline__ void each_group(const float *xr, const float *xor_, const float *gr, const float *cr, int64_t D, int groups,
                                           const float (&rx)[kSampleElems], const float (&ro)[kSampleElems],
                                           const float (&rg)[kSampleElems], const float (&rc)[kSampleElems], F body) {
    if (RES) {
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) {
            const float xv[4] = {rx[g * 4], rx[g * 4 + 1], rx[g * 4 + 2], rx[g * 4 + 3]};
            const float ov[4] = {ro[g * 4], ro[g * 4 + 1], ro[g * 4 + 2], ro[g * 4 + 3]};
            const float gv[4] = {rg[g * 4], rg[g * 4 + 1], rg[g * 4 + 2], rg[g * 4 + 3]};
            const float cv[4] = {rc[g * 4], rc[g * 4 + 1], rc[g * 4 + 2], rc[g * 4 + 3]};
            body(group_element(g), xv, ov, gv, cv);
        }
    } else {
        for (int g = 0; g < groups; ++g) {
            const int64_t e = group_element(g);
            float xv[4], ov[4], gv[4], cv[4];
            load4<VEC>(xr, e, D, xv);
            load4<VEC>(xor_, e, D, ov);
            load4<VEC>(gr, e, D, gv);
            load4<VEC>(cr, e, D, cv);
            body(e, xv, ov, gv, cv);
        }
    }
}

template <bool RES, bool VEC>
__global__ __launch_bounds__(kSampleBlock) void step_l2_kernel(float *x, float *x_old, const float *__restrict__ g,
                                                               const float *__restrict__ x0, const float *__restrict__ step,
                                                               const int *__restrict__ counter, float *__restrict__ norms, int64_t B, int64_t D,
                                                               float eps) {
    __shared__ double sh[2 * kSampleWaves];
    SampleReducer red{sh};
    const int64_t b = blockIdx.x;
    float *xr = x + b * D, *xor_ = x_old + b * D;
    const float *gr = g + b * D, *cr = x0 + b * D;
    const int groups = groups_of(D);
    const float a = counter[0] == 0 ? 1.0f : 0.75f;
    L2Op op{a, 1.0f - a, eps, false, 0.0f, 0.0f, 0.0f};

    // pass 1: ||g||; the resident path takes the sample into registers here
    float rx[kSampleElems], ro[kSampleElems], rg[kSampleElems], rc[kSampleElems];
    double acc = 0.0;
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            const int64_t e = group_element(k);
            float xv[4], ov[4], gv[4], cv[4];
            load4<VEC>(xr, e, D, xv);
            load4<VEC>(xor_, e, D, ov);
            load4<VEC>(gr, e, D, gv);
            load4<VEC>(cr, e, D, cv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double v = static_cast<double>(gv[j]);
                acc += v * v;
                rx[k * 4 + j] = xv[j], ro[k * 4 + j] = ov[j], rg[k * 4 + j] = gv[j], rc[k * 4 + j] = cv[j];
            }
        }
    } else {
        for (int k = 0; k < groups; ++k) {
            float gv[4];
            load4<VEC>(gr, group_element(k), D, gv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double v = static_cast<double>(gv[j]);
                acc += v * v;
            }
        }
    }
    const float ng = static_cast<float>(sqrt(red.sum(acc)));
    op.take = isfinite(ng);  // uniform over the workgroup
    op.sg = step[b] / (ng + kTiny);

    // pass 2: ||z - x0|| after the gradient step
    acc = 0.0;
    each_group<RES, VEC>(xr, xor_, gr, cr, D, groups, rx, ro, rg, rc,
                         [&](int64_t, const float(&xv)[4], const float(&)[4], const float(&gv)[4], const float(&cv)[4]) {
#pragma unroll
                             for (int j = 0; j < 4; ++j) {
                                 const double v = static_cast<double>(op.d1(xv[j], gv[j], cv[j]));
                                 acc += v * v;
                             }
                         });
    const float n1 = static_cast<float>(sqrt(red.sum(acc)));
    op.s1 = rescale(eps, n1);

    // pass 3: ||m - x0|| after the momentum mix
    acc = 0.0;
    each_group<RES, VEC>(xr, xor_, gr, cr, D, groups, rx, ro, rg, rc,
                         [&](int64_t, const float(&xv)[4], const float(&ov)[4], const float(&gv)[4], const float(&cv)[4]) {
#pragma unroll
                             for (int j = 0; j < 4; ++j) {
                                 const double v = static_cast<double>(op.d2(xv[j], ov[j], gv[j], cv[j]));
                                 acc += v * v;
                             }
                         });
    const float n2 = static_cast<float>(sqrt(red.sum(acc)));
    op.s2 = rescale(eps, n2);
    if (threadIdx.x == 0) norms[b] = ng, norms[B + b] = n1, norms[2 * B + b] = n2;

    // final pass: the one place x and x_old are written, each element by the thread that read it
    each_group<RES, VEC>(xr, xor_, gr, cr, D, groups, rx, ro, rg, rc,
                         [&](int64_t e, const float(&xv)[4], const float(&ov)[4], const float(&gv)[4], const float(&cv)[4]) {
                             float r[4];
#pragma unroll
                             for (int j = 0; j < 4; ++j) r[j] = op.next(xv[j], ov[j], gv[j], cv[j]);
                             store4<VEC>(xor_, e, D, xv);
                             store4<VEC>(xr, e, D, r);
                         });
}

}  // namespace

EE_API int ee_apgd_step_l2_f32(float *x, float *x_old, const float *g, const float *x0, const float *step, const int *counter, float *norms,
                               int64_t B, int64_t per_sample, float eps, int path, void *stream) {
    if (B < 0 || per_sample < 0 || B > INT32_MAX || per_sample > INT32_MAX || (per_sample > 0 && B > INT64_MAX / per_sample)) return EE_ERR_SHAPE;
    if (!(eps >= 0.0f)) return EE_ERR_SHAPE;
    bool res;
    if (const int rc = sample_path(path, per_sample, &res)) return rc;
    if (B == 0 || per_sample == 0) return EE_OK;
    if (!x || !x_old || !g || !x0 || !step || !counter || !norms) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(x_old) || !aligned4(g) || !aligned4(x0) || !aligned4(step) || !aligned4(counter) || !aligned4(norms))
        return EE_ERR_ALIGN;
    sample_launch(res, sample_vec(per_sample, x, x_old, g, x0), [&](auto RES, auto VEC) {
        EE_LAUNCH((step_l2_kernel<RES, VEC>), dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), x, x_old, g, x0, step,
                  counter, norms, B, per_sample, eps);
    });
    return launch_status();
}
