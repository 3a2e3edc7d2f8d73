// ee_sqatk_l2.hip - the Square attack in the L2 threat model (Andriushchenko et al. 2020, Alg. 3): the two launches that
// stand in the place of ee_sqatk_init_f32 and ee_sqatk_step_f32 in an L2 run.  The margin launch, the counter, the flags and the query
// count do not know the norm (ee_sqatk.hip).
//
// Start, per sample, with eta0 = the [s0, s0] table, tiny = 1e-12f - every operation rounded once in f32:
//     d   = +-eta0 (or its transpose) on each of the nh x nw tiles, sign per (tile, channel), transpose per tile; 0 outside the tiling
//     n0  = ||d||_2        q = eps / (n0 + tiny)        x_best = x_new = clamp(x0 + d * q, 0, 1)
// Proposal i, per sample, with s = sizes[i], eta = the table at eta_off[i], W1 / W2 the two s x s windows, delta = x_best - x0:
//     n_img = ||delta||_2        n_un = ||delta on W1 u W2||_2        n_w[c] = ||delta[c, W1]||_2
//     new[c]   = +-eta + delta[c, W1] / (tiny + n_w[c])                            n_new[c] = ||new[c]||_2
//     scale    = sqrt(max(eps * eps - n_img * n_img, 0) / C + n_un * n_un)
//     delta[:, W2] = 0;   delta[c, W1] = new[c] / (tiny + n_new[c]) * scale          n_d = ||delta||_2
//     x_new    = clamp(x0 + delta / (tiny + n_d) * eps, 0, 1)
//
// One workgroup per sample: the norms depend on each other in three rounds ({n_img, n_un, n_w}, {n_new}, {n_d}) and never cross a
// workgroup.  The first two rounds are propose_window's (ee_sqatk_prop.hpp) under the policy below; this file adds round 3 and the last
// pass.  A norm is (float) sqrt(S), S the sum of the squares in double (the square of a float is exact there) in the one order of
// ee_sample.hpp; the Reducer takes a round's sums together and adds each one's eight partials in that index order.  An element
// outside a window adds an exact zero to that window's sum (or is skipped, which is the same number), so the order depends on the shape
// only and the resident path (x0, the difference and what is known of each element stay in registers across the rounds), the streaming
// path (every pass re-reads x_best and x0 and recomputes from the scalars already known) and the vector / element-wise accesses all
// return the same bits.
// flags[b] and margin_min[b] are read by sample b's workgroup only and are uniform in it.  x_best is written in the first pass only
// (the commit), x_new in the last, each element by the thread that read it.
#include <math.h>

#include "ee_sqatk_prop.hpp"

namespace {

using namespace ee;

// the L2 norm of propose_window
struct NormL2 {
    static constexpr int kHead = 3;  // n_img, n_un, n_d
    static __device__ __forceinline__ double term(float v) {
        const double d = static_cast<double>(v);
        return d * d;
    }
    static __device__ __forceinline__ float fin(double s) { return static_cast<float>(sqrt(s)); }
    static __device__ __forceinline__ float scale(float eps, float n_img, float n_un, int C) {
        const float room = tmax(eps * eps - n_img * n_img, 0.0f);
        return static_cast<float>(sqrt(static_cast<double>(room / static_cast<float>(C) + n_un * n_un)));  // the f32 root, rounded once
    }
};

// ---- start ---------------------------------------------------------------------------------------------------------------------------
template <bool RES, bool VEC>
__global__ __launch_bounds__(kSampleBlock) void init_l2_kernel(float *__restrict__ x_best, float *__restrict__ x_new, const float *__restrict__ x0,
                                                           const int64_t *__restrict__ seed, const float *__restrict__ eta, int s0, int C, int H,
                                                           int W, float eps) {
    __shared__ double part[kSampleWaves];
    __shared__ float sn[1];
    Reducer red{part};
    const Geo geo{C, H, W, H * W, static_cast<int64_t>(C) * H * W};
    const int64_t b = blockIdx.x, D = geo.D;
    const float *cr = x0 + b * D;
    float *br = x_best + b * D, *nr = x_new + b * D;
    const int groups = groups_of(D);
    const Tiling tl(seed, eta, s0, H, W, b);

    float rc[kSampleElems], rd[kSampleElems];
    double acc = 0.0;
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            const int64_t e = group_element(k);
            float cv[4], dv[4];
            load4<VEC>(cr, e, D, cv);
            tl.d4(e, geo, dv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rc[k * 4 + j] = cv[j], rd[k * 4 + j] = dv[j];
                acc += NormL2::term(rd[k * 4 + j]);
            }
        }
    } else {
        for (int k = 0; k < groups; ++k) {
            float dv[4];
            tl.d4(group_element(k), geo, dv);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += NormL2::term(dv[j]);
        }
    }
    red.put(0, acc);
    red.sums(1, sn, nullptr, 0, 0, [](int k) { return k; }, NormL2::fin);
    const float q = eps / (sn[0] + kTiny);
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = tclamp(rc[k * 4 + j] + rd[k * 4 + j] * q, 0.0f, 1.0f);
            store4<VEC>(br, group_element(k), D, o);
            store4<VEC>(nr, group_element(k), D, o);
        }
    } else {
        for (int k = 0; k < groups; ++k) {
            const int64_t e = group_element(k);
            float cv[4], dv[4], o[4];
            load4<VEC>(cr, e, D, cv);
            tl.d4(e, geo, dv);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = tclamp(cv[j] + dv[j] * q, 0.0f, 1.0f);
            store4<VEC>(br, e, D, o);
            store4<VEC>(nr, e, D, o);
        }
    }
}

// ---- commit and proposal -------------------------------------------------------------------------------------------------------------
template <bool RES, bool VEC>
__global__ __launch_bounds__(kSampleBlock) void step_l2_kernel(float *x_best, float *x_new, const float *__restrict__ x0, const int *__restrict__ flags,
                                                           const float *__restrict__ margin_min, const int *__restrict__ counter,
                                                           const int *__restrict__ sizes, const int *__restrict__ eta_off,
                                                           const float *__restrict__ eta, int n_sizes, const int64_t *__restrict__ seed,
                                                           float *__restrict__ norms, int64_t B, int C, int H, int W, float eps) {
    __shared__ double part[(2 + kMaxC) * kSampleWaves];
    __shared__ float sn1[2 + kMaxC], sn2[kMaxC], sn3[1];
    Reducer red{part};
    Proposal p;
    Stream<VEC> stream;
    float rc[kSampleElems], rv[kSampleElems];
    Info ri[kSampleElems];
    const StepArgs a{x_best, x_new, x0, flags, margin_min, counter, sizes, eta_off, eta, n_sizes, seed, norms, B, C, H, W, eps};
    if (!propose_window<NormL2, RES, VEC>(a, red, sn1, sn2, p, stream, rc, rv, ri)) return;
    const int64_t b = blockIdx.x, D = stream.geo.D;
    float *nr = x_new + b * D;
    const int groups = groups_of(D);
    const auto all = [](const Info(&)[4]) { return true; };

    // round 3: n_d over the whole sample
    double a_d = 0.0;
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) {
            rv[k] = p.stage2(rv[k], ri[k]);
            a_d += NormL2::term(rv[k]);
        }
    } else {
        for (int k = 0; k < groups; ++k)
            stream(k, all, [&](int64_t, const float(&)[4], const float(&dv)[4], const Info(&in)[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) a_d += NormL2::term(p.stage2(p.stage1(dv[j], in[j]), in[j]));
            });
    }
    red.put(0, a_d);
    red.sums(1, sn3, norms, B, b, [](int) { return 2; }, NormL2::fin);
    const float n_d = sn3[0];
    // the L2 run's last line: the whole delta rescaled to the sphere
    const auto next = [&](float x0v, float v) { return tclamp(x0v + v / (kTiny + n_d) * eps, 0.0f, 1.0f); };

    // final pass: the one place x_new is written
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = next(rc[k * 4 + j], rv[k * 4 + j]);
            store4<VEC>(nr, group_element(k), D, o);
        }
    } else {
        for (int k = 0; k < groups; ++k)
            stream(k, all, [&](int64_t e, const float(&cv)[4], const float(&dv)[4], const Info(&in)[4]) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = next(cv[j], p.stage2(p.stage1(dv[j], in[j]), in[j]));
                store4<VEC>(nr, e, D, o);
            });
    }
}

// what both entry points check of (B, C, H, W, eps, path); *res: the resident path runs
int check_l2(int B, int C, int H, int W, float eps, int path, bool *res) {
    const int rc = sqatk_check_shape(B, C, H, W);
    if (rc != EE_OK) return rc;
    if (!(eps >= 0.0f)) return EE_ERR_SHAPE;
    return sample_path(path, static_cast<int64_t>(C) * H * W, res);
}

}  // namespace

EE_API int ee_sqatk_init_l2_f32(float *x_best, float *x_new, const float *x0, const int64_t *seed, const float *eta, int s0, int B, int C, int H,
                                int W, float eps, int path, void *stream) {
    bool res = false;
    int rc = check_l2(B, C, H, W, eps, path, &res);
    if (rc != EE_OK) return rc;
    if (s0 < 1 || s0 > H || s0 > W) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if ((rc = sqatk_check_ptrs(seed, {x_best, x_new, x0, eta})) != EE_OK) return rc;
    ProfScope prof(EE_K_SQATK_INIT, as_stream(stream));
    sample_launch(res, sample_vec(static_cast<int64_t>(C) * H * W, x_best, x_new, x0), [&](auto RES, auto VEC) {
        EE_LAUNCH((init_l2_kernel<RES, VEC>), dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), x_best, x_new, x0, seed,
                  eta, s0, C, H, W, eps);
    });
    return launch_status();
}

EE_API int ee_sqatk_step_l2_f32(float *x_best, float *x_new, const float *x0, const int *flags, const float *margin_min, const int *counter,
                                const int *sizes, const int *eta_off, const float *eta, int n_sizes, const int64_t *seed, float *norms, int B,
                                int C, int H, int W, float eps, int path, void *stream) {
    bool res = false;
    int rc = check_l2(B, C, H, W, eps, path, &res);
    if (rc != EE_OK) return rc;
    if (n_sizes < 0) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if ((rc = sqatk_check_ptrs(seed, {x_best, x_new, x0, flags, margin_min, counter, norms}, n_sizes > 0, {sizes, eta_off, eta})) != EE_OK) return rc;
    const int64_t Bl = B;
    ProfScope prof(EE_K_SQATK_STEP, as_stream(stream));
    sample_launch(res, sample_vec(static_cast<int64_t>(C) * H * W, x_best, x_new, x0), [&](auto RES, auto VEC) {
        EE_LAUNCH((step_l2_kernel<RES, VEC>), dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), x_best, x_new, x0, flags,
                  margin_min, counter, sizes, eta_off, eta, n_sizes, seed, norms, Bl, C, H, W, eps);
    });
    return launch_status();
}
