// ee_apgd_l1.hip - APGD in the L1 threat model (Croce & Hein 2021, "Mind the box: l1-APGD for sparse adversarial attacks on image
// classifiers"): the sparse sign step, the exact Euclidean projection onto {z : ||z - x0||_1 <= eps} n [0,1]^D, and the checkpoint rule
// that adapts a per-sample sparsity and step size.  Losses and copies do not know the norm (ee_apgd_loss_f32, ee_apgd_select_f32).
//
// The step, per sample (no momentum), every f32 operation rounded once:
//     j   = clamp((int) floorf((1 - topk) * (float) D), 0, D - 1)        tau = the j-th smallest |g_i| (0-based; ordered by bit pattern)
//     m   = #{i : |g_i| >= tau, g_i < 0 or g_i > 0}                      sg  = step / ((float) m + 1e-10f)
//     u_i = x_i + sg * sign(g_i) where |g_i| >= tau, else x_i            (u = x when g holds a NaN or an Inf: no gradient step)
//     x   = P(u)
// The projection P(u), per coordinate w = u - x0, a = |w|, s = sign(w), lo = min(max(0, -min(1 - u, u)), a):
//     z = clamp(x0 + s * (a - min(max(lambda, lo), a)), 0, 1)
// lambda = 0 when h(0) <= eps, else the root of h(lambda) = sum_i (a_i - min(max(lambda, lo_i), a_i)) = eps.  h is continuous, piecewise
// linear and non-increasing with the 2D non-negative breakpoints {lo_i} u {a_i}.  The kernel finds T, the largest float with h(T) > eps, by
// 31 steps over the bit pattern of non-negative floats (one workgroup-wide sum each) and solves the segment (T, T+] (T+ the next float:
// no breakpoint lies strictly inside) in closed form over A = {i : lo_i <= T < a_i}:
//     lambda = (sum_{lo_i > T} (a_i - lo_i) + sum_A a_i - eps) / |A|,        rounded to float and kept inside [T, T+]
// - the segment solve of the sort-based formulation, not a bisection stopped at a tolerance; |A| = 0 takes T+.  tau comes from the same kind
// of search on integers: the largest pattern T with #{|g_i| < T} <= j.
//
// One workgroup per sample in all three launches, so no launch writes a per-sample scalar that another workgroup of that launch reads.
// Counts are integer sums, real sums are double (differences of two floats are exact there) in the one order of ee_sample.hpp, which the
// resident path (a sample stays in registers across all passes) and the streaming path (every pass re-reads its inputs and recomputes u
// from tau and sg) share, so the two return the same bits.  Every loop has a trip count fixed by per_sample and the launch shape; the
// branches around the searches are taken on values the whole workgroup holds alike.
// The output is written in the final pass only, each element by the thread that read it.
// The projection itself - coordinate, search, segment solve, final pass - is ee_l1_proj.hpp's, shared with ee_sqatk_l1.hip.
#include <math.h>

#include "ee_l1_proj.hpp"

namespace {

using namespace ee;

// the sparse sign step of one element; the scalars are filled in as they become known
struct L1StepOp {
    bool take;     // the gradient is finite everywhere: the step is taken
    uint32_t tau;  // bit pattern of the threshold
    float sg;
    __device__ __forceinline__ float operator()(float x, float g) const {
        const float s = sgn(g);  // a zero entry rests whatever sg is (m = 0 makes sg step * 1e10, which may overflow)
        return (take && s != 0.0f && abs_bits(g) >= tau) ? x + sg * s : x;
    }
};

// the gradient of every element of the thread, in the same order on both paths (zeros past D)
template <bool RES, bool VEC, class F>
__device__ __forceinline__ void each_g(const float *gr, int64_t D, int groups, const float (&rg)[kSampleElems], F body) {
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) body(rg[k]);
    } else {
        for (int g = 0; g < groups; ++g) {
            float gv[4];
            load4<VEC>(gr, group_element(g), D, gv);
#pragma unroll
            for (int j = 0; j < 4; ++j) body(gv[j]);
        }
    }
}

// (element, w = u - x0, lo, x0) of every float4 group of the thread, in the same order on both paths (zeros past D).  RES: the groups
// live in rw / rl / rc.  Otherwise every pass re-reads its rows; a step launch (STEP) recomputes u from x and g.
template <bool RES, bool VEC, bool STEP, class F>
__device__ __forceinline__ void each_c(const float *ur, const float *gr, const float *cr, int64_t D, int groups, const L1StepOp &op,
                                       const float (&rw)[kSampleElems], const float (&rl)[kSampleElems], const float (&rc)[kSampleElems],
                                       F body) {
    if (RES) {
        l1_each_resident(rw, rl, rc, body);
    } else {
        for (int g = 0; g < groups; ++g) {
            const int64_t e = group_element(g);
            float uv[4], cv[4];
            load4<VEC>(ur, e, D, uv);
            load4<VEC>(cr, e, D, cv);
            if (STEP) {
                float gv[4];
                load4<VEC>(gr, e, D, gv);
#pragma unroll
                for (int j = 0; j < 4; ++j) uv[j] = op(uv[j], gv[j]);
            }
            float wv[4], lv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const L1Coord c = L1Coord::of(uv[j], cv[j]);
                wv[j] = c.w, lv[j] = c.lo;
            }
            body(e, wv, lv, cv);
        }
    }
}

// STEP: z == u_in is x (in place), g the gradient; scal [7, B].  Otherwise the projection alone: u_in -> z, g unused; scal [4, B].
template <bool RES, bool VEC, bool STEP>
__global__ __launch_bounds__(kSampleBlock) void l1_kernel(float *z, const float *u_in, const float *g, const float *x0, const float *step,
                                                      const float *topk, float *scal, int64_t B, int64_t D, float eps) {
    __shared__ double shd[2 * kSampleWaves];
    __shared__ int shi[2 * kSampleWaves];
    SampleReducer red{shd, shi};
    const int64_t b = blockIdx.x;
    float *zr = z + b * D;
    const float *ur = u_in + b * D, *cr = x0 + b * D;
    const float *gr = STEP ? g + b * D : nullptr;
    const int groups = groups_of(D);
    const int64_t pad = static_cast<int64_t>(RES ? kSampleVecs : groups) * kSampleSlots - D;  // slots past D: they read as zeros

    float ru[kSampleElems], rg[kSampleElems], rc[kSampleElems], rl[kSampleElems];  // ru: x, then u, then w = u - x0
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            const int64_t e = group_element(k);
            float uv[4], cv[4], gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            load4<VEC>(ur, e, D, uv);
            load4<VEC>(cr, e, D, cv);
            if (STEP) load4<VEC>(gr, e, D, gv);
#pragma unroll
            for (int j = 0; j < 4; ++j) ru[k * 4 + j] = uv[j], rc[k * 4 + j] = cv[j], rg[k * 4 + j] = gv[j];
        }
    }

    L1StepOp op{false, 0u, 0.0f};
    int jsel = 0, m = 0;
    if (STEP) {
        // j from topk[b]; a NaN or negative product selects 0
        const float v = (1.0f - topk[b]) * static_cast<float>(D);
        const float fl = floorf(v);
        jsel = !(fl >= 0.0f) ? 0 : (fl >= static_cast<float>(D) ? static_cast<int>(D - 1) : static_cast<int>(fl));
        if (jsel > D - 1) jsel = static_cast<int>(D - 1);
        // tau: the largest pattern T with #{|g_i| < T} <= j.  The slots past D hold |g| = 0 and are below every candidate: `pad` takes them out.
        uint32_t T = 0u;
#pragma unroll 1
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            int c = 0;
            each_g<RES, VEC>(gr, D, groups, rg, [&](float gv) { c += abs_bits(gv) < cand ? 1 : 0; });
            if (static_cast<int64_t>(red.sum(c)) - pad <= static_cast<int64_t>(jsel)) T = cand;
        }
        int cm = 0, cn = 0;
        each_g<RES, VEC>(gr, D, groups, rg, [&](float gv) {
            cm += (abs_bits(gv) >= T && (gv < 0.0f || gv > 0.0f)) ? 1 : 0;
            cn += abs_bits(gv) >= 0x7F800000u ? 1 : 0;
        });
        m = red.sum(cm);
        op.take = red.sum(cn) == 0;  // uniform over the workgroup
        op.tau = T;
        op.sg = step[b] / (static_cast<float>(m) + 1e-10f);
        if (RES) {
#pragma unroll
            for (int k = 0; k < kSampleElems; ++k) ru[k] = op(ru[k], rg[k]);
        }
    }

    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) {
            const L1Coord c = L1Coord::of(ru[k], rc[k]);
            ru[k] = c.w, rl[k] = c.lo;
        }
    }
    // the projection of u (ee_l1_proj.hpp)
    const auto each = [&](auto body) { each_c<RES, VEC, STEP>(ur, gr, cr, D, groups, op, ru, rl, rc, body); };
    const L1Root root = l1_root(red, eps, each);
    const double dist = l1_write(red, root, each, [&](int64_t e, const float(&r)[4]) { store4<VEC>(zr, e, D, r); });
    if (threadIdx.x == 0) {
        l1_scal(scal, B, b, root, dist);
        if (STEP) {
            scal[4 * B + b] = __uint_as_float(op.tau);
            scal[5 * B + b] = static_cast<float>(m);
            scal[6 * B + b] = static_cast<float>(jsel);
        }
    }
}

// ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kSampleBlock) void book_l1_kernel(const float *__restrict__ loss, const int *__restrict__ pred,
                                                           const float *__restrict__ x, const float *__restrict__ x_best,
                                                           const float *__restrict__ x0, float *fstate, int *istate, float *topk, int *spstate,
                                                           const int *__restrict__ counter, const int *__restrict__ sched, int n_iter,
                                                           int64_t B, int64_t D, float eps) {
    __shared__ double shd[2 * kSampleWaves];
    __shared__ int shi[2 * kSampleWaves];
    SampleReducer red{shd, shi};
    const int64_t b = blockIdx.x;
    float *step = fstate + EE_APGD_F_STEP * B, *loss_best = fstate + EE_APGD_F_LOSS_BEST * B;
    int *robust = istate + EE_APGD_I_ROBUST * B, *flags = istate + EE_APGD_I_FLAGS * B;
    int *sp_old = spstate, *sp_last = spstate + B;
    const int it = counter[0];
    const int k = (it >= 0 && it < n_iter) ? sched[it] : 0;  // window length when a checkpoint closes this iteration, else 0
    // every thread reads the sample's scalars; thread 0 writes them behind the barrier below
    const float l = loss[b], best = loss_best[b], st = step[b];
    const int pr = pred[b], spo = sp_old[b];
    const bool improved = l > best;
    int sp = 0;
    if (k > 0) {  // uniform over the launch: the schedule decides it, not the data
        const float *vr = (improved ? x : x_best) + b * D, *cr = x0 + b * D;
        const int groups = groups_of(D);
        int c = 0;
        for (int g = 0; g < groups; ++g) {
            const int64_t e = group_element(g);
            float vv[4], cv[4];
            load4<VEC>(vr, e, D, vv);
            load4<VEC>(cr, e, D, cv);
#pragma unroll
            for (int j = 0; j < 4; ++j) c += vv[j] != cv[j] ? 1 : 0;
        }
        sp = red.sum(c);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int f = 0;
    if (!pr) {
        robust[b] = 0;
        f |= EE_APGD_FOOLED;
    }
    if (improved) {
        loss_best[b] = l;
        f |= EE_APGD_IMPROVED;
    }
    if (k > 0) {
        const bool reduced = (static_cast<float>(sp) / static_cast<float>(spo)) < 0.95f;
        topk[b] = static_cast<float>(sp) / static_cast<float>(D) / 1.5f;
        const float s = reduced ? eps : st / 1.5f;
        step[b] = fminf(fmaxf(s, eps / 10.0f), eps);
        sp_old[b] = sp;
        sp_last[b] = sp;
        if (reduced) f |= EE_APGD_REDUCED;
    }
    flags[b] = f;
}

// what the projection and the step check of (B, per_sample, eps, path); *res: the resident path runs
int check_l1(int64_t B, int64_t per_sample, float eps, int path, bool *res) {
    // per_sample plus the padded slots of the last float4 group must fit the integer counts of a pass
    if (B < 0 || per_sample < 0 || B > INT32_MAX || per_sample > INT32_MAX - kSampleSlots || (per_sample > 0 && B > INT64_MAX / per_sample))
        return EE_ERR_SHAPE;
    if (!(eps >= 0.0f)) return EE_ERR_SHAPE;
    return sample_path(path, per_sample, res);
}

template <bool STEP>
int launch_l1(float *z, const float *u, const float *g, const float *x0, const float *step, const float *topk, float *scal, int64_t B,
              int64_t per_sample, float eps, bool res, void *stream) {
    const bool vec = sample_vec(per_sample, z, u, x0) && (!STEP || aligned16(g));
    sample_launch(res, vec, [&](auto RES, auto VEC) {
        EE_LAUNCH((l1_kernel<RES, VEC, STEP>), dim3(static_cast<unsigned>(B)), dim3(kSampleBlock), 0, as_stream(stream), z, u, g, x0, step, topk,
                  scal, B, per_sample, eps);
    });
    return launch_status();
}

}  // namespace

EE_API int ee_l1_proj_f32(float *z, const float *u, const float *x0, float *scal, int64_t B, int64_t per_sample, float eps, int path,
                          void *stream) {
    bool res;
    if (const int rc = check_l1(B, per_sample, eps, path, &res)) return rc;
    if (B == 0 || per_sample == 0) return EE_OK;
    if (!z || !u || !x0 || !scal) return EE_ERR_NULL;
    if (!aligned4(z) || !aligned4(u) || !aligned4(x0) || !aligned4(scal)) return EE_ERR_ALIGN;
    return launch_l1<false>(z, u, nullptr, x0, nullptr, nullptr, scal, B, per_sample, eps, res, stream);
}

EE_API int ee_apgd_step_l1_f32(float *x, const float *g, const float *x0, const float *step, const float *topk, float *scal, int64_t B,
                               int64_t per_sample, float eps, int path, void *stream) {
    bool res;
    if (const int rc = check_l1(B, per_sample, eps, path, &res)) return rc;
    if (B == 0 || per_sample == 0) return EE_OK;
    if (!x || !g || !x0 || !step || !topk || !scal) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(g) || !aligned4(x0) || !aligned4(step) || !aligned4(topk) || !aligned4(scal)) return EE_ERR_ALIGN;
    return launch_l1<true>(x, x, g, x0, step, topk, scal, B, per_sample, eps, res, stream);
}

EE_API int ee_apgd_book_l1_f32(const float *loss, const int *pred, const float *x, const float *x_best, const float *x0, float *fstate,
                               int *istate, float *topk, int *spstate, const int *counter, const int *sched, int n_iter, int64_t B,
                               int64_t per_sample, float eps, void *stream) {
    if (B < 0 || per_sample < 0 || B > INT32_MAX || per_sample > INT32_MAX - kSampleSlots || n_iter < 1 || !(eps >= 0.0f)) return EE_ERR_SHAPE;
    if (B == 0 || per_sample == 0) return EE_OK;
    if (!loss || !pred || !x || !x_best || !x0 || !fstate || !istate || !topk || !spstate || !counter || !sched) return EE_ERR_NULL;
    if (!aligned4(loss) || !aligned4(pred) || !aligned4(x) || !aligned4(x_best) || !aligned4(x0) || !aligned4(fstate) || !aligned4(istate) ||
        !aligned4(topk) || !aligned4(spstate) || !aligned4(counter) || !aligned4(sched))
        return EE_ERR_ALIGN;
    const dim3 grid(static_cast<unsigned>(B)), block(kSampleBlock);
    if (sample_vec(per_sample, x, x_best, x0))
        EE_LAUNCH(book_l1_kernel<true>, grid, block, 0, as_stream(stream), loss, pred, x, x_best, x0, fstate, istate, topk, spstate, counter,
                  sched, n_iter, B, per_sample, eps);
    else
        EE_LAUNCH(book_l1_kernel<false>, grid, block, 0, as_stream(stream), loss, pred, x, x_best, x0, fstate, istate, topk, spstate, counter,
                  sched, n_iter, B, per_sample, eps);
    return launch_status();
}
