// ee_pert.hip - the perturbation check of an evaluation: what utils/aa.py prints after a run.
//     ee_pert_check_f32   per sample: Linf, L2 and L1 of d = x_adv - x0, the range of x_adv and its NaN count
// One workgroup of 512 threads per sample (ee_sample.hpp), one pass over the two rows.  It reads no host value that changes, allocates
// nothing and synchronises nothing; a workgroup writes the scalars of its own sample only and reads none.
#include <math.h>

#include "ee_sample.hpp"

namespace {

using namespace ee;

// Per element, each operation rounded once in the order written: d = x_adv - x0 (f32), a = |d|.  Over the sample, in the one order of
// ee_sample.hpp:  S2 = sum d^2 and S1 = sum a in double (the square of a float and a float itself are exact there), M = max a,
// hi = max x_adv, lo = min x_adv (fmax / fmin: a NaN entry is skipped; no entry at all leaves -inf / +inf), n = #{x_adv is NaN}.
// Elements at or past D read as 0 in both rows - d = 0 adds nothing to a sum and cannot raise M - and are kept out of hi, lo and n.
// A NaN in d (a NaN in either row, or inf - inf) makes S1 NaN, and only that does: the terms are non-negative.  The three norms are then
// NaN.  RES loads the whole sample into registers before the first reduction (24 + 24 values per thread); the streaming path reduces
// as it reads.  Both add the same terms in the same order.
struct Acc {
    double s2 = 0.0, s1 = 0.0, m = 0.0, hi = -INFINITY, nlo = -INFINITY;  // nlo = max(-x_adv) = -min(x_adv): one max reduction serves both
    int nan = 0;
    __device__ __forceinline__ void add(const float (&xa)[4], const float (&x0)[4], int64_t e, int64_t D) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = xa[j] - x0[j];
            const double a = static_cast<double>(fabsf(d));
            s2 = fma(a, a, s2);
            s1 += a;
            m = fmax(m, a);
            if (e + j < D) {
                const double v = static_cast<double>(xa[j]);
                hi = fmax(hi, v);
                nlo = fmax(nlo, -v);
                nan += xa[j] != xa[j];
            }
        }
    }
};

template <bool RES, bool VEC>
__global__ __launch_bounds__(kSampleBlock) void pert_kernel(const float *__restrict__ x_adv, const float *__restrict__ x0, int64_t D,
                                                            float *__restrict__ norms, float *__restrict__ range, int *__restrict__ n_nan) {
    const int b = blockIdx.x;
    const int64_t off = static_cast<int64_t>(b) * D;
    const float *ar = x_adv + off, *x0r = x0 + off;
    __shared__ double shd[2 * kSampleWaves];
    __shared__ int shi[2 * kSampleWaves];
    SampleReducer red{shd, shi};
    Acc acc;
    if (RES) {
        float ka[kSampleVecs][4], k0[kSampleVecs][4];
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) {
            load4<VEC>(ar, group_element(g), D, ka[g]);
            load4<VEC>(x0r, group_element(g), D, k0[g]);
        }
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) acc.add(ka[g], k0[g], group_element(g), D);
    } else {
        const int groups = groups_of(D);
        for (int g = 0; g < groups; ++g) {
            float a4[4], o4[4];
            load4<VEC>(ar, group_element(g), D, a4);
            load4<VEC>(x0r, group_element(g), D, o4);
            acc.add(a4, o4, group_element(g), D);
        }
    }
    const double s2 = red.sum(acc.s2), s1 = red.sum(acc.s1);
    const double m = red.max(acc.m), hi = red.max(acc.hi), nlo = red.max(acc.nlo);
    const int nan = red.sum(acc.nan);
    if (threadIdx.x == 0) {
        const bool bad = s1 != s1;
        norms[3 * b + 0] = bad ? NAN : static_cast<float>(m);
        norms[3 * b + 1] = bad ? NAN : static_cast<float>(sqrt(s2));
        norms[3 * b + 2] = bad ? NAN : static_cast<float>(s1);
        range[2 * b + 0] = static_cast<float>(-nlo);
        range[2 * b + 1] = static_cast<float>(hi);
        n_nan[b] = nan;
    }
}

bool bad_shape(int64_t B, int64_t per_sample) {
    return B < 0 || per_sample < 1 || B > INT32_MAX / 4 || per_sample > INT32_MAX || B > INT64_MAX / per_sample;
}

}  // namespace

EE_API int ee_pert_check_f32(const float *x_adv, const float *x0, int64_t B, int64_t per_sample, float *norms, float *range, int *n_nan,
                             int path, void *stream) {
    if (bad_shape(B, per_sample)) return EE_ERR_SHAPE;
    bool resident;
    if (const int rc = sample_path(path, per_sample, &resident)) return rc;
    if (B == 0) return EE_OK;
    if (!x_adv || !x0 || !norms || !range || !n_nan) return EE_ERR_NULL;
    if (!aligned4(x_adv) || !aligned4(x0) || !aligned4(norms) || !aligned4(range) || !aligned4(n_nan)) return EE_ERR_ALIGN;
    ProfScope prof(EE_K_PGD_STEP, as_stream(stream));
    const dim3 grid(static_cast<unsigned>(B)), block(kSampleBlock);
    sample_launch(resident, sample_vec(per_sample, x_adv, x0), [&](auto RES, auto VEC) {
        EE_LAUNCH((pert_kernel<RES, VEC>), grid, block, 0, as_stream(stream), x_adv, x0, per_sample, norms, range, n_nan);
    });
    return launch_status();
}
