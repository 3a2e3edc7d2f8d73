// ee_apgd.hip - the hot path of APGD (Croce & Hein 2020, "standard" version, Linf): the momentum step with a per-sample step size, the
// per-row losses (CE, DLR, targeted DLR) with their logit gradients, the per-sample bookkeeping, and the tensor copies it decides.
//
// One iteration is four launches around the classifier:
//     ee_apgd_step_f32    x, x_old <- momentum step            (element-wise, 128-bit accesses, reads step[b] and the iteration counter)
//     ee_apgd_loss_f32    logits -> row loss, dlogits, pred    (one wavefront per row, ee_rows.hpp)
//     ee_apgd_book_f32    per-sample scalars -> flags          (one thread per sample; the checkpoint comes from sched[counter])
//     ee_apgd_select_f32  copies under the flags, counter += 1 (element-wise; a sample without a flag costs the flag read)
// Nothing here depends on a host value that changes from iteration to iteration, so one captured graph serves every iteration.
// No launch writes a per-sample scalar (or the counter) that another thread of the same launch reads: book owns row b's scalars in
// thread b alone and only reads the counter; select only reads the flags and is the one place that advances the counter.
#include <math.h>

#include "ee_rows.hpp"

namespace {

using namespace ee;

// ---- step ----------------------------------------------------------------------------------------------------------------------------
struct StepOp {
    float a, eps;
    // returns x_new; the caller stores x as the new x_old
    __device__ __forceinline__ float operator()(float x, float xo, float g, float x0, float step) const {
        const float z = proj_linf(x + step * sgn(g), x0, eps);
        return proj_linf((x + (z - x) * a) + (x - xo) * (1.0f - a), x0, eps);
    }
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void step_kernel(float *x, float *x_old, const float *__restrict__ g, const float *__restrict__ x0,
                                                      const float *__restrict__ step, const int *__restrict__ counter, int64_t n,
                                                      int64_t per_sample, float eps) {
    const StepOp op{counter[0] == 0 ? 1.0f : 0.75f, eps};
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (VEC == 4) {
        const int64_t nv = n >> 2;
        for (int64_t v = i; v < nv; v += stride) {
            const float4 vx = reinterpret_cast<const float4 *>(x)[v];
            const float4 vo = reinterpret_cast<const float4 *>(x_old)[v];
            const float4 vg = reinterpret_cast<const float4 *>(g)[v];
            const float4 v0 = reinterpret_cast<const float4 *>(x0)[v];
            // per_sample need not be a multiple of 4: the four elements may belong to up to four samples
            const int64_t base = v << 2;
            int64_t b = base / per_sample;
            int64_t left = per_sample - (base - b * per_sample);  // elements of sample b from `base` on (>= 1)
            float s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (left == 0) {
                    ++b;
                    left = per_sample;
                }
                s[k] = step[b];  // base + k < n, so b < B
                --left;
            }
            float4 r;
            r.x = op(vx.x, vo.x, vg.x, v0.x, s[0]);
            r.y = op(vx.y, vo.y, vg.y, v0.y, s[1]);
            r.z = op(vx.z, vo.z, vg.z, v0.z, s[2]);
            r.w = op(vx.w, vo.w, vg.w, v0.w, s[3]);
            reinterpret_cast<float4 *>(x_old)[v] = vx;
            reinterpret_cast<float4 *>(x)[v] = r;
        }
        for (int64_t k = (nv << 2) + i; k < n; k += stride) {
            const float xv = x[k];
            const float r = op(xv, x_old[k], g[k], x0[k], step[k / per_sample]);
            x_old[k] = xv;
            x[k] = r;
        }
    } else {
        for (int64_t k = i; k < n; k += stride) {
            const float xv = x[k];
            const float r = op(xv, x_old[k], g[k], x0[k], step[k / per_sample]);
            x_old[k] = xv;
            x[k] = r;
        }
    }
}

// ---- losses --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void loss_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                      const int64_t *__restrict__ targets, int B, int K, int kind,
                                                      float *__restrict__ row_loss, float *__restrict__ dlogits, int *__restrict__ pred) {
    const int lane = threadIdx.x & (kWave - 1);
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= B) return;
    const float *z = logits + static_cast<size_t>(row) * K;
    float *d = dlogits + static_cast<size_t>(row) * K;
    const int64_t y64 = labels[row], t64 = kind == EE_APGD_DLR_T ? targets[row] : 0;
    if (y64 < 0 || y64 >= K || t64 < 0 || t64 >= K) {  // a label outside the row is never dereferenced: NaN loss, no gradient, not "correct"
        for (int k = lane; k < K; k += kWave) d[k] = 0.0f;
        if (lane == 0) {
            row_loss[row] = NAN;
            pred[row] = 0;
        }
        return;
    }
    const int y = static_cast<int>(y64), t = static_cast<int>(t64);
    if (kind == EE_APGD_CE) {
        int pi[1];
        float pv[1];
        row_top<1>(z, K, lane, pi, pv);
        float mx, lse;  // ee_ce_f32's loss and gradient: loss = lse - (z_y - max)
        row_stats(z, K, lane, mx, lse);
        for (int k = lane; k < K; k += kWave) d[k] = ce_grad(z[k], mx, lse, k == y, 1.0f);
        if (lane == 0) {
            row_loss[row] = lse - (z[y] - mx);
            pred[row] = pi[0] == y;
        }
        return;
    }
    int pi[4] = {kNone, kNone, kNone, kNone};
    float pv[4];
    int o;      // the class subtracted from z_y
    float den;  // the spread that normalises the margin
    if (kind == EE_APGD_DLR) {
        int qi[3];
        float qv[3];
        row_top<3>(z, K, lane, qi, qv);
        pi[0] = qi[0], pi[1] = qi[1], pi[2] = qi[2];
        pv[0] = qv[0], pv[1] = qv[1], pv[2] = qv[2];
        o = pi[0] == y ? pi[1] : pi[0];
        den = (pv[0] - pv[2]) + 1e-12f;
    } else {
        row_top<4>(z, K, lane, pi, pv);
        o = t;
        // z_p1 - (z_p3 + z_p4)/2 as the mean of the two differences z_p1 - z_p3 and z_p1 - z_p4 (both >= 0, each rounded once, their sum
        // does not cancel).  Subtracting the rounded sum instead cancels when the spread is small against the logits: 2.5e-6 relative
        // in a 3*randn row of 1000 classes.  The host path keeps the other order, so its fp32 loss differs in the last bits.
        den = ((pv[0] - pv[2]) + (pv[0] - pv[3])) * 0.5f + 1e-12f;
    }
    const float num = z[y] - z[o];
    const float inv = 1.0f / den, den2 = den * den, slope = num / den2;  // -d loss / d num, d loss / d den
    // up to five (class, coefficient) pairs.  DLR: the label coincides with p1 or p3 in most rows and the two contributions nearly cancel
    // there (-1/d + n/d^2 with n ~ d), so those sums are formed analytically: d + n and n - d are single differences of logits.
    int ci[5] = {-1, -1, -1, -1, -1};
    float cv[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (kind == EE_APGD_DLR) {
        if (pi[0] == y) {  // o = p2:  y: -1/d + n/d^2 = -((z_p2 - z_p3) + 1e-12)/d^2
            ci[0] = y, cv[0] = -((pv[1] - pv[2]) + 1e-12f) / den2;
            ci[1] = pi[1], cv[1] = inv;
            ci[2] = pi[2], cv[2] = -slope;
        } else {  // o = p1:  p1: 1/d + n/d^2 = ((z_y - z_p3) + 1e-12)/d^2
            ci[0] = pi[0], cv[0] = ((z[y] - pv[2]) + 1e-12f) / den2;
            if (y == pi[2]) {  // y: -1/d - n/d^2 = -1e-12/d^2
                ci[1] = y, cv[1] = -1e-12f / den2;
            } else {
                ci[1] = y, cv[1] = -inv;
                ci[2] = pi[2], cv[2] = -slope;
            }
        }
    } else {
        ci[0] = y, cv[0] = -inv;
        ci[1] = t, cv[1] = inv;
        ci[2] = pi[0], cv[2] = slope;
        ci[3] = pi[2], cv[3] = -slope * 0.5f;
        ci[4] = pi[3], cv[4] = -slope * 0.5f;
    }
    for (int k = lane; k < K; k += kWave) {
        float v = 0.0f;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (k == ci[j]) v += cv[j];
        d[k] = v;
    }
    if (lane == 0) {
        row_loss[row] = -(num / den);
        pred[row] = pi[0] == y;
    }
}

// ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void book_kernel(const float *__restrict__ loss, const int *__restrict__ pred, float *fstate, int *istate,
                                                      const int *__restrict__ counter, const int *__restrict__ sched, int n_iter, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float *step = fstate + static_cast<size_t>(EE_APGD_F_STEP) * B, *loss_best = fstate + static_cast<size_t>(EE_APGD_F_LOSS_BEST) * B;
    float *f_prev = fstate + static_cast<size_t>(EE_APGD_F_PREV) * B, *best_last = fstate + static_cast<size_t>(EE_APGD_F_LOSS_BEST_LAST) * B;
    int *inc = istate + static_cast<size_t>(EE_APGD_I_INC) * B, *reduced_last = istate + static_cast<size_t>(EE_APGD_I_REDUCED_LAST) * B;
    int *robust = istate + static_cast<size_t>(EE_APGD_I_ROBUST) * B, *flags = istate + static_cast<size_t>(EE_APGD_I_FLAGS) * B;
    const int it = counter[0];
    const int k = (it >= 0 && it < n_iter) ? sched[it] : 0;  // window length when a checkpoint closes this iteration, else 0
    const float l = loss[b];
    int f = 0;
    if (!pred[b]) {
        robust[b] = 0;
        f |= EE_APGD_FOOLED;
    }
    int c = inc[b] + (l > f_prev[b] ? 1 : 0);
    f_prev[b] = l;
    float best = loss_best[b];
    if (l > best) {
        best = l;
        loss_best[b] = l;
        f |= EE_APGD_IMPROVED;
    }
    if (k > 0) {
        const bool osc = 4 * c <= 3 * k;
        const bool noimp = !reduced_last[b] && (best_last[b] >= best);
        const bool red = osc || noimp;
        reduced_last[b] = red ? 1 : 0;
        best_last[b] = best;
        c = 0;
        if (red) {
            step[b] = step[b] * 0.5f;
            f |= EE_APGD_REDUCED;
        }
    }
    inc[b] = c;
    flags[b] = f;
}

// ---- copies --------------------------------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kBlock) void select_kernel(float *x, float *g, float *x_best, float *g_best, float *x_best_adv,
                                                        const int *__restrict__ flags, int *counter, int64_t per_sample) {
    const int b = blockIdx.x;
    if (b == 0 && blockIdx.y == 0 && threadIdx.x == 0) counter[0] = counter[0] + 1;  // nobody reads the counter in this launch
    const int f = flags[b];
    if (f == 0) return;
    const bool fooled = f & EE_APGD_FOOLED, improved = f & EE_APGD_IMPROVED;
    const bool restore = (f & EE_APGD_REDUCED) && !improved;  // improved and reduced: x is x_best already
    const int64_t off = static_cast<int64_t>(b) * per_sample;
    const int64_t stride = static_cast<int64_t>(gridDim.y) * blockDim.x;
    const int64_t i = static_cast<int64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
    if (VEC == 4) {  // per_sample % 4 == 0 and 16-byte bases: a sample is a whole number of aligned vectors
        float4 *vx = reinterpret_cast<float4 *>(x + off), *vg = reinterpret_cast<float4 *>(g + off);
        float4 *vxb = reinterpret_cast<float4 *>(x_best + off), *vgb = reinterpret_cast<float4 *>(g_best + off);
        float4 *vxa = reinterpret_cast<float4 *>(x_best_adv + off);
        for (int64_t v = i; v < (per_sample >> 2); v += stride) {
            if (fooled || improved) {  // steps (5) and (7) see the iterate, step (8) then replaces it
                const float4 xv = vx[v];
                if (fooled) vxa[v] = xv;
                if (improved) {
                    vxb[v] = xv;
                    vgb[v] = vg[v];
                }
            }
            if (restore) {
                vx[v] = vxb[v];
                vg[v] = vgb[v];
            }
        }
    } else {
        for (int64_t k = i; k < per_sample; k += stride) {
            const int64_t e = off + k;
            if (fooled || improved) {
                const float xv = x[e];
                if (fooled) x_best_adv[e] = xv;
                if (improved) {
                    x_best[e] = xv;
                    g_best[e] = g[e];
                }
            }
            if (restore) {
                x[e] = x_best[e];
                g[e] = g_best[e];
            }
        }
    }
}

}  // namespace

EE_API int ee_apgd_step_f32(float *x, float *x_old, const float *g, const float *x0, const float *step, const int *counter, int64_t B,
                            int64_t per_sample, float eps, void *stream) {
    if (B < 0 || per_sample < 0 || (per_sample > 0 && B > INT64_MAX / per_sample)) return EE_ERR_SHAPE;
    const int64_t n = B * per_sample;
    if (n == 0) return EE_OK;
    if (!x || !x_old || !g || !x0 || !step || !counter) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(x_old) || !aligned4(g) || !aligned4(x0) || !aligned4(step) || !aligned4(counter)) return EE_ERR_ALIGN;
    const bool vec = aligned16(x) && aligned16(x_old) && aligned16(g) && aligned16(x0);
    const unsigned blocks = grid_for(vec ? (n + 3) / 4 : n);
    if (vec)
        EE_LAUNCH(step_kernel<4>, dim3(blocks), dim3(kBlock), 0, as_stream(stream), x, x_old, g, x0, step, counter, n,
                  per_sample, eps);
    else
        EE_LAUNCH(step_kernel<1>, dim3(blocks), dim3(kBlock), 0, as_stream(stream), x, x_old, g, x0, step, counter, n,
                  per_sample, eps);
    return launch_status();
}

EE_API int ee_apgd_loss_f32(const float *logits, const int64_t *labels, const int64_t *targets, int B, int K, int kind, float *row_loss,
                            float *dlogits, int *pred, void *stream) {
    if (B < 0 || K < 1 || K > 65536 || kind < EE_APGD_CE || kind > EE_APGD_DLR_T) return EE_ERR_SHAPE;
    if ((kind == EE_APGD_DLR && K < 3) || (kind == EE_APGD_DLR_T && K < 4)) return EE_ERR_UNSUPPORTED;
    if (B == 0) return EE_OK;
    if (!logits || !labels || !row_loss || !dlogits || !pred || (kind == EE_APGD_DLR_T && !targets)) return EE_ERR_NULL;
    EE_LAUNCH(loss_kernel, dim3(row_grid(B)), dim3(kBlock), 0, as_stream(stream), logits,
              labels, targets, B, K, kind, row_loss, dlogits, pred);
    return launch_status();
}

EE_API int ee_apgd_book_f32(const float *loss, const int *pred, float *fstate, int *istate, const int *counter, const int *sched, int n_iter,
                            int B, void *stream) {
    if (B < 0 || n_iter < 1) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!loss || !pred || !fstate || !istate || !counter || !sched) return EE_ERR_NULL;
    if (!aligned4(loss) || !aligned4(pred) || !aligned4(fstate) || !aligned4(istate) || !aligned4(counter) || !aligned4(sched)) return EE_ERR_ALIGN;
    EE_LAUNCH(book_kernel, dim3(static_cast<unsigned>((B + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), loss, pred, fstate,
              istate, counter, sched, n_iter, B);
    return launch_status();
}

EE_API int ee_apgd_select_f32(float *x, float *g, float *x_best, float *g_best, float *x_best_adv, const int *flags, int *counter, int B,
                              int64_t per_sample, void *stream) {
    if (B < 0 || per_sample < 0) return EE_ERR_SHAPE;
    if (B == 0 || per_sample == 0) return EE_OK;  // an empty batch is no attack: nothing is launched, the counter stays
    if (!x || !g || !x_best || !g_best || !x_best_adv || !flags || !counter) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(g) || !aligned4(x_best) || !aligned4(g_best) || !aligned4(x_best_adv) || !aligned4(flags) || !aligned4(counter))
        return EE_ERR_ALIGN;
    const bool vec = (per_sample & 3) == 0 && aligned16(x) && aligned16(g) && aligned16(x_best) && aligned16(g_best) && aligned16(x_best_adv);
    const int64_t work = vec ? per_sample / 4 : per_sample;
    int64_t chunks = (work + kBlock - 1) / kBlock;
    if (chunks > 64) chunks = 64;
    const dim3 grid(static_cast<unsigned>(B), static_cast<unsigned>(chunks));
    if (vec)
        EE_LAUNCH(select_kernel<4>, grid, dim3(kBlock), 0, as_stream(stream), x, g, x_best, g_best, x_best_adv, flags, counter, per_sample);
    else
        EE_LAUNCH(select_kernel<1>, grid, dim3(kBlock), 0, as_stream(stream), x, g, x_best, g_best, x_best_adv, flags, counter, per_sample);
    return launch_status();
}
