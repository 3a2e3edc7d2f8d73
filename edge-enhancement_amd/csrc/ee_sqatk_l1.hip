// ee_sqatk_l1.hip - the Square attack in the L1 threat model (Croce & Hein 2021, "Mind the box"): the two launches
// that stand in the place of ee_sqatk_init_f32 and ee_sqatk_step_f32 in an L1 run.  The margin launch, the counter, the flags and the
// query count do not know the norm (ee_sqatk.hip); pattern, windows, draws and the window-1 update are the L2 run's by construction - the
// step is propose_window (ee_sqatk_prop.hpp) under the policy below, then the projection, which is ee_l1_proj_f32's (ee_l1_proj.hpp).
//
// eps is the L1 radius, eps_p <= eps the radius every projection uses (the host forms it).  P_r(u) is the Euclidean projection onto
// {z : ||z - x0||_1 <= r} n [0,1]^D.  tiny = 1e-12f - every operation rounded once in f32:
// Start, per sample, with eta0 = the [s0, s0] table:
//     d   = +-eta0 (or its transpose) on each of the nh x nw tiles, sign per (tile, channel), transpose per tile; 0 outside the tiling
//     u   = x0 + d        x_best = x_new = P_{eps_p}(u)
// Proposal i, per sample, with s = sizes[i], eta = the table at eta_off[i], W1 / W2 the two s x s windows, delta = x_best - x0:
//     n_img = ||delta||_1        n_un = ||delta on W1 u W2||_1        n_w[c] = ||delta[c, W1]||_1
//     new[c]   = +-eta + delta[c, W1] / (tiny + n_w[c])                            n_new[c] = ||new[c]||_1
//     scale    = max(eps - n_img, 0) / C + n_un
//     delta[:, W2] = 0;   delta[c, W1] = new[c] / (tiny + n_new[c]) * scale
//     u = x0 + delta      x_new = P_{eps_p}(u)
//
// One workgroup per sample.  A norm is (float) S, S the sum of the |values| in double (exact there) in the one order of ee_sample.hpp; the
// Reducer takes a round's sums ({n_img, n_un, n_w}, then {n_new}) together.  An element outside a window adds an exact zero to that
// window's sum, so the order depends on the shape only, and the resident path, the streaming path and the vector / element-wise accesses
// all return the same bits.  On the resident path the proposal keeps (x0, the value, what is known of the element) in registers and hands
// (x0, w = u - x0, lo) to the projection; the streaming path recomputes a coordinate from x_best, x0 and the scalars in every pass.
// A sample that makes no proposal runs no projection: P of a point of the set is not the identity in bits.
// flags[b] and margin_min[b] are read by sample b's workgroup only and are uniform in it.  x_best is written in the first pass only
// (the commit), x_new in the last, each element by the thread that read it.
#include <math.h>

#include "ee_l1_proj.hpp"
#include "ee_sqatk_prop.hpp"

namespace {

using namespace ee;

// the L1 norm of propose_window
struct NormL1 {
    static constexpr int kHead = 2;  // n_img, n_un
    static __device__ __forceinline__ double term(float v) { return fabs(static_cast<double>(v)); }
    static __device__ __forceinline__ float fin(double s) { return static_cast<float>(s); }
    static __device__ __forceinline__ float scale(float eps, float n_img, float n_un, int C) {
        return tmax(eps - n_img, 0.0f) / static_cast<float>(C) + n_un;
    }
};

// (w, lo) of u = x0 + v, four at a time
__device__ __forceinline__ void coords4(const float (&cv)[4], const float (&vv)[4], float (&wv)[4], float (&lv)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const L1Coord c = L1Coord::of(cv[j] + vv[j], cv[j]);
        wv[j] = c.w, lv[j] = c.lo;
    }
}

// ---- start ---------------------------------------------------------------------------------------------------------------------------
template <bool RES, bool VEC>
__global__ __launch_bounds__(kSampleBlock) void init_l1_kernel(float *__restrict__ x_best, float *__restrict__ x_new, const float *__restrict__ x0,
                                                           const int64_t *__restrict__ seed, const float *__restrict__ eta, int s0,
                                                           float *__restrict__ scal, int64_t B, int C, int H, int W, float eps_p) {
    __shared__ double shd[2 * kSampleWaves];
    __shared__ int shi[2 * kSampleWaves];
    SampleReducer red{shd, shi};
    const Geo geo{C, H, W, H * W, static_cast<int64_t>(C) * H * W};
    const int64_t b = blockIdx.x, D = geo.D;
    const float *cr = x0 + b * D;
    float *br = x_best + b * D, *nr = x_new + b * D;
    const int groups = groups_of(D);
    const Tiling tl(seed, eta, s0, H, W, b);
    const auto group = [&](int64_t e, float (&cv)[4], float (&wv)[4], float (&lv)[4]) {
        float dv[4];
        load4<VEC>(cr, e, D, cv);
        tl.d4(e, geo, dv);
        coords4(cv, dv, wv, lv);
    };

    float rc[kSampleElems], rw[kSampleElems], rl[kSampleElems];
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            float cv[4], wv[4], lv[4];
            group(group_element(k), cv, wv, lv);
#pragma unroll
            for (int j = 0; j < 4; ++j) rc[k * 4 + j] = cv[j], rw[k * 4 + j] = wv[j], rl[k * 4 + j] = lv[j];
        }
    }
    const auto each = [&](auto body) {
        if (RES) {
            l1_each_resident(rw, rl, rc, body);
        } else {
            for (int k = 0; k < groups; ++k) {
                const int64_t e = group_element(k);
                float cv[4], wv[4], lv[4];
                group(e, cv, wv, lv);
                body(e, wv, lv, cv);
            }
        }
    };
    const L1Root root = l1_root(red, eps_p, each);
    const double dist = l1_write(red, root, each, [&](int64_t e, const float(&r)[4]) {
        store4<VEC>(br, e, D, r);
        store4<VEC>(nr, e, D, r);
    });
    if (threadIdx.x == 0) l1_scal(scal, B, b, root, dist);
}

// ---- commit and proposal -------------------------------------------------------------------------------------------------------------
template <bool RES, bool VEC>
__global__ __launch_bounds__(kSampleBlock) void step_l1_kernel(float *x_best, float *x_new, const float *__restrict__ x0, const int *__restrict__ flags,
                                                           const float *__restrict__ margin_min, const int *__restrict__ counter,
                                                           const int *__restrict__ sizes, const int *__restrict__ eta_off,
                                                           const float *__restrict__ eta, int n_sizes, const int64_t *__restrict__ seed,
                                                           float *__restrict__ norms, float *__restrict__ scal, int64_t B, int C, int H, int W,
                                                           float eps, float eps_p) {
    __shared__ double part[(2 + kMaxC) * kSampleWaves];
    __shared__ float sn1[2 + kMaxC], sn2[kMaxC];
    __shared__ double shd[2 * kSampleWaves];
    __shared__ int shi[2 * kSampleWaves];
    Reducer rnd{part};
    SampleReducer red{shd, shi};
    Proposal p;
    Stream<VEC> stream;
    float rc[kSampleElems], rv[kSampleElems], rl[kSampleElems];  // rv: delta, then new, then w = u - x0; rl: lo, the projection's alone
    Info ri[kSampleElems];                                       // the proposal's alone
    const StepArgs a{x_best, x_new, x0, flags, margin_min, counter, sizes, eta_off, eta, n_sizes, seed, norms, B, C, H, W, eps};
    const int64_t b = blockIdx.x, D = static_cast<int64_t>(C) * H * W;
    if (!propose_window<NormL1, RES, VEC>(a, rnd, sn1, sn2, p, stream, rc, rv, ri)) {  // no proposal, no projection: its rows are zeros
        if (threadIdx.x < 4) scal[static_cast<int64_t>(threadIdx.x) * B + b] = 0.0f;
        return;
    }
    float *nr = x_new + b * D;
    const int groups = groups_of(D);

    // u = x0 + delta and its projection: from here on the resident path holds (x0, w, lo) and what is known of an element is dead
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) {
            const L1Coord c = L1Coord::of(rc[k] + p.stage2(rv[k], ri[k]), rc[k]);
            rv[k] = c.w, rl[k] = c.lo;
        }
    }
    const auto each = [&](auto body) {
        if (RES) {
            l1_each_resident(rv, rl, rc, body);
        } else {
            for (int k = 0; k < groups; ++k)
                stream(k, [](const Info(&)[4]) { return true; }, [&](int64_t e, const float(&cv)[4], const float(&dv)[4], const Info(&in)[4]) {
                    float vv[4], wv[4], lv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) vv[j] = p.stage2(p.stage1(dv[j], in[j]), in[j]);
                    coords4(cv, vv, wv, lv);
                    body(e, wv, lv, cv);
                });
        }
    };
    const L1Root root = l1_root(red, eps_p, each);
    // final pass: the one place x_new is written
    const double dist = l1_write(red, root, each, [&](int64_t e, const float(&r)[4]) { store4<VEC>(nr, e, D, r); });
    if (threadIdx.x == 0) l1_scal(scal, B, b, root, dist);
}

// what both entry points check of (B, C, H, W, eps, eps_p, path); *res: the resident path runs
int check_sq_l1(int B, int C, int H, int W, float eps, float eps_p, int path, bool *res) {
    const int rc = sqatk_check_shape(B, C, H, W);
    if (rc != EE_OK) return rc;
    if (!(eps >= 0.0f) || !(eps_p >= 0.0f) || !(eps_p <= eps)) return EE_ERR_SHAPE;
    // the padded slots of the last float4 group must fit the integer counts of a projection pass
    if (static_cast<int64_t>(C) * H * W > INT32_MAX - kSampleSlots) return EE_ERR_SHAPE;
    return sample_path(path, static_cast<int64_t>(C) * H * W, res);
}

}  // namespace

EE_API int ee_sqatk_init_l1_f32(float *x_best, float *x_new, const float *x0, const int64_t *seed, const float *eta, int s0, float *scal,
                                int B, int C, int H, int W, float eps, float eps_p, int path, void *stream) {
    bool res = false;
    int rc = check_sq_l1(B, C, H, W, eps, eps_p, path, &res);
    if (rc != EE_OK) return rc;
    if (s0 < 1 || s0 > H || s0 > W) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if ((rc = sqatk_check_ptrs(seed, {x_best, x_new, x0, eta, scal})) != EE_OK) return rc;
    const int64_t Bl = B;
    ProfScope prof(EE_K_SQATK_INIT, as_stream(stream));
    sample_launch(res, sample_vec(static_cast<int64_t>(C) * H * W, x_best, x_new, x0), [&](auto RES, auto VEC) {
        EE_LAUNCH((init_l1_kernel<RES, VEC>), dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), x_best, x_new, x0, seed,
                  eta, s0, scal, Bl, C, H, W, eps_p);
    });
    return launch_status();
}

EE_API int ee_sqatk_step_l1_f32(float *x_best, float *x_new, const float *x0, const int *flags, const float *margin_min, const int *counter,
                                const int *sizes, const int *eta_off, const float *eta, int n_sizes, const int64_t *seed, float *norms,
                                float *scal, int B, int C, int H, int W, float eps, float eps_p, int path, void *stream) {
    bool res = false;
    int rc = check_sq_l1(B, C, H, W, eps, eps_p, path, &res);
    if (rc != EE_OK) return rc;
    if (n_sizes < 0) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if ((rc = sqatk_check_ptrs(seed, {x_best, x_new, x0, flags, margin_min, counter, norms, scal}, n_sizes > 0, {sizes, eta_off, eta})) != EE_OK)
        return rc;
    const int64_t Bl = B;
    ProfScope prof(EE_K_SQATK_STEP, as_stream(stream));
    sample_launch(res, sample_vec(static_cast<int64_t>(C) * H * W, x_best, x_new, x0), [&](auto RES, auto VEC) {
        EE_LAUNCH((step_l1_kernel<RES, VEC>), dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), x_best, x_new, x0, flags,
                  margin_min, counter, sizes, eta_off, eta, n_sizes, seed, norms, scal, Bl, C, H, W, eps, eps_p);
    });
    return launch_status();
}
