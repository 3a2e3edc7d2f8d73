// ee_fab.hip - the hot path of FAB-T (Croce & Hein 2020, "Minimally distorted adversarial examples with a fast adaptive boundary attack";
// Linf, targeted, the constants of AutoAttack's "standard" version: eta = 1.05, beta = 0.9, alpha_max = 0.1, one run, no random start).
// One iteration is four launches around two forwards and one backward of the classifier:
//     ee_fab_diff_f32       logits -> df = z_t - z_y, its logit gradient, pred        (one wavefront per row, as ee_apgd_loss_f32)
//     ee_fab_proj_linf_f32  (x, x0, w, df) -> lambda, sign, ||delta||_inf of the two box-constrained Linf projections of a sample
//                           (one workgroup per problem, 2B problems; scalars only - the two deltas never reach memory)
//     ee_fab_step_f32       rebuilds delta1 / delta2 per element from those scalars, mixes, writes the new x   (element-wise, 128-bit accesses)
//     ee_fab_commit_f32     after the second forward: argmax, ||x - x0||_inf, adv / res update, the shrink step, counter += 1
//                           (one workgroup per sample)
// Nothing here depends on a host value that changes from iteration to iteration, so one captured graph serves every iteration.  No launch
// writes a per-sample scalar that another workgroup of the same launch reads: a projection problem and a commit sample each belong to one
// workgroup, step only reads the scalars, and commit is the one place that advances the counter (nothing reads it there).
//
// The threat model (Linf; L2; L1, section 20) enters at three launches and nothing else - the projection, the step
// that rebuilds its deltas, and the commit's distance ||x - x0|| (in double in the same order for L2 and L1): ee_fab_proj_{linf,l2,l1}_f32,
// ee_fab_step{,_l2,_l1}_f32, ee_fab_commit{,_l2,_l1}_f32, each one template on the Metric.  ee_fab_diff_f32 is shared.
//
// The projection.  For v = s w (s the sign of c), c' = |c| and rooms r_i (the distance of p_i to the bound v_i pushes it to), the least-norm
// delta onto the hyperplane inside the box is fixed by one scalar, the root of a monotone piecewise function of it:
//     Linf  delta_i = -sign(v_i) min(lambda, r_i)      g(lambda) = sum_i |v_i| min(lambda, r_i) = c',        breakpoints r_i
//     L2    delta_i = -sign(v_i) min(mu |v_i|, r_i)    g(mu) = sum_i |v_i| min(mu |v_i|, r_i) = c',          breakpoints t_i = r_i / |v_i|
//     L1    a fractional-knapsack fill by descending |v_i|: F(T) = sum_{|v_i| >= T} |v_i| r_i is a non-increasing step function, theta the
//           largest float with F(theta) >= c'; coordinates above theta go to their bounds, those AT theta all take the same fraction
//           phi = (c' - sum_{|v_i| > theta} |v_i| r_i) / sum_{|v_i| = theta} |v_i| r_i of their rooms
// Each kernel finds T, the largest float on the near side of the root, by 31 steps over the bit pattern of non-negative floats (one
// workgroup-wide sum each, no sort), and then solves the segment that contains the root in closed form - lambda = (c' - sum_{r_i <= T}
// |v_i| r_i) / sum_{r_i > T} |v_i|, mu = (c' - sum_{t_i <= T} |v_i| r_i) / sum_{t_i > T} v_i^2, phi as above.  No breakpoint lies strictly
// between T and the root, so this IS the segment solve of the sort-based formulation - not a bisection stopped at a tolerance - and every
// loop has a trip count fixed by D and the launch shape.  All sums are double (products of two floats are exact there) in the one order of
// ee_sample.hpp, which the resident path (a problem's |w_i| and r_i stay in registers across all passes) and the streaming path (re-read
// through L2) share, so the two return the same bits.
//
// Untargeted FAB keeps all of the above and changes where w and df come from: per iteration one forward, then per
// class k one backward pass (the logit gradient from ee_fab_diff_f32 with targets = k) and one ee_fab_select_f32 - the dual norm of that
// class's gradient, dist = |z_k - z_y| / (1e-12 + n), and a running arg-min per sample that keeps (dist, k, df, the row) of the closest
// linearised boundary.  One streaming pass and, on improvement, a copy; the reset before class 0 is a `first` flag of the same launch.
//
// Restarts add one launch outside the iteration, ee_fab_start_f32: the random point at distance min(res, eps) / 2
// from x0 that restart r >= 1 begins at - from injected noise or from Philox, in the metric of the run.  The captured graph does not see it.
#include <math.h>

#include "ee_sample.hpp"

namespace {

using namespace ee;

constexpr float kEta = 1.05f, kBeta = 0.9f, kAlphaMax = 0.1f;

enum Metric : int { kLinf = 0, kL2 = 1, kL1 = 2 };  // EE_FAB_METRIC_*: the instances of every kernel and launch below that has an M

// the room of a coordinate at p that v pushes down (v > 0: to 0) or up (v < 0: to 1); 0 where v is 0 or NaN.  Never negative.
__device__ __forceinline__ float room(float v, float p) { return fmaxf(v > 0.0f ? p : (v < 0.0f ? 1.0f - p : 0.0f), 0.0f); }

// ---- df, its logit gradient, pred ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void diff_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                      const int64_t *__restrict__ targets, int B, int K, float *__restrict__ df,
                                                      float *__restrict__ dlogits, int *__restrict__ pred) {
    const int lane = threadIdx.x & (kWave - 1);
    const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= B) return;
    const float *z = logits + static_cast<size_t>(row) * K;
    float *d = dlogits + static_cast<size_t>(row) * K;
    const int64_t y = labels[row], t = targets[row];
    const bool valid = y >= 0 && y < K && t >= 0 && t < K;  // a label or target outside the row is never dereferenced
    bool nan;
    const int first = row_first(z, K, lane, nan);
    for (int k = lane; k < K; k += kWave) d[k] = valid ? (k == t ? 1.0f : 0.0f) - (k == y ? 1.0f : 0.0f) : 0.0f;
    if (lane == 0) {
        df[row] = valid ? z[t] - z[y] : NAN;
        pred[row] = first;
    }
}

// ---- the projection ------------------------------------------------------------------------------------------------------------------
// One workgroup per problem: problem b projects x[b] with c = df[b], problem B + b projects x0[b] with c = df[b] + <w[b], x0[b] - x[b]>.
// proj_begin and each_element are what the three metrics share - the indexing, pass 1, the two degenerate exits and (|w|, room) of every
// element in the one order of ee_sample.hpp - and solve_linf / solve_l2 / solve_l1 below are what they do not.

// The L2 breakpoint of a coordinate: the f32 quotient, rounded once - the one definition both paths (and the host path) classify by.  A
// denormal |v_i| overflows it to +inf: that coordinate never saturates.  |v_i| = 0 (its room is 0 too) gives 0: the coordinate counts as
// saturated from the start and adds exact zeros, so no pass ever forms inf * 0.
__device__ __forceinline__ float ratio(float a, float r) { return a != 0.0f ? r / a : 0.0f; }

struct Problem {
    const float *wr, *pr;  // the rows of w and of the point this problem projects
    int64_t D;
    int groups;
    float s, cp;  // of a live problem: the sign of c and c' = |c|; v = s w
};

// RES: groups 0 .. kSampleVecs-1 of this thread live in a[] / r[] (zeros past D); otherwise every pass re-reads w and p.  BRK (L2): the
// breakpoint goes with them - the resident path keeps t[] next to a[] / r[] (no division in the 33 passes), the streaming path recomputes
// it from what it re-reads; without BRK t[] has one element that nothing touches.
template <bool BRK>
using Breaks = float[BRK ? kSampleElems : 1];

// False: the problem is degenerate and rest(on_the_hyperplane) has written its rows.  Every thread of the workgroup returns the same, so
// the caller's early exit is uniform.
template <bool RES, bool VEC, bool BRK, class Rest>
__device__ __forceinline__ bool proj_begin(const float *__restrict__ x, const float *__restrict__ x0, const float *__restrict__ w,
                                                const float *__restrict__ df, int B, int64_t D, SampleReducer &red, Problem &p,
                                                float (&a)[kSampleElems], float (&r)[kSampleElems], Breaks<BRK> &t, Rest rest) {
    const int q = blockIdx.x, b = q < B ? q : q - B;
    const bool second = q >= B;  // problem B + b projects x0, problem b projects x
    const float *xr = x + static_cast<int64_t>(b) * D, *x0r = x0 + static_cast<int64_t>(b) * D, *wr = w + static_cast<int64_t>(b) * D;
    p.wr = wr, p.pr = second ? x0r : xr, p.D = D, p.groups = groups_of(D);

    // pass 1: sum |w_i| and sum w_i (x0_i - x_i); the resident path keeps w in a[] and the point in r[]
    double sabs = 0.0, dot = 0.0;
    auto first = [&](int g) {
        const int64_t e = group_element(g);
        float wv[4], xv[4], ov[4];
        load4<VEC>(wr, e, D, wv);
        load4<VEC>(xr, e, D, xv);
        load4<VEC>(x0r, e, D, ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sabs += static_cast<double>(fabsf(wv[j]));
            dot = fma(static_cast<double>(wv[j]), static_cast<double>(ov[j] - xv[j]), dot);
            if (RES) {
                a[g * 4 + j] = wv[j];
                r[g * 4 + j] = second ? ov[j] : xv[j];
            }
        }
    };
    if (RES) {
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) first(g);
    } else {
        for (int g = 0; g < p.groups; ++g) first(g);
    }
    sabs = red.sum(sabs);
    dot = red.sum(dot);
    const float d = df[b];
    // every decision below is taken on values all threads of the workgroup hold alike
    if (!(isfinite(d) && d != 0.0f && isfinite(sabs) && sabs > 0.0)) {  // no hyperplane to project onto: both problems of the sample rest
        rest(false);
        return false;
    }
    const float c = second ? static_cast<float>(static_cast<double>(d) + dot) : d;
    const float s = c >= 0.0f ? 1.0f : -1.0f;  // NaN cannot come here: d and dot are finite
    p.s = s, p.cp = fabsf(c);
    if (!isfinite(c) || p.cp == 0.0f) {  // c = 0: the point lies on the hyperplane
        rest(true);
        return false;
    }
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) {
            const float wv = a[k];
            r[k] = room(s * wv, r[k]);
            a[k] = fabsf(wv);
            if (BRK) t[k] = ratio(a[k], r[k]);
        }
    }
    return true;
}

// body(|w|, room) - with BRK body(|w|, room, breakpoint) - of every element of the thread, in the same order on both paths
template <bool RES, bool VEC, bool BRK, class F>
__device__ __forceinline__ void each_element(const Problem &p, const float (&a)[kSampleElems], const float (&r)[kSampleElems],
                                             const Breaks<BRK> &t, F body) {
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) {
            if constexpr (BRK)
                body(a[k], r[k], t[k]);
            else
                body(a[k], r[k]);
        }
    } else {
        for (int g = 0; g < p.groups; ++g) {
            const int64_t e = group_element(g);
            float wv[4], pv[4];
            load4<VEC>(p.wr, e, p.D, wv);
            load4<VEC>(p.pr, e, p.D, pv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float av = fabsf(wv[j]), rv = room(p.s * wv[j], pv[j]);
                if constexpr (BRK)
                    body(av, rv, ratio(av, rv));
                else
                    body(av, rv);
            }
        }
    }
}

// ---- Linf: lambda, the smallest value with g(lambda) = sum_i |v_i| min(lambda, r_i) = c' ---------------------------------------------------
template <class Each>
__device__ __forceinline__ void solve_linf(Each each, const Problem &p, SampleReducer &red, float *lam_out, float *sgn_out, float *nrm_out) {
    // g(inf) and the largest room among the coordinates that move
    double ginf = 0.0, rm = 0.0;
    each([&](float av, float rv) {
        ginf = fma(static_cast<double>(av), static_cast<double>(rv), ginf);
        if (av != 0.0f) rm = fmax(rm, static_cast<double>(rv));
    });
    ginf = red.sum(ginf);
    const float rmax = static_cast<float>(red.max(rm));
    const double cpd = static_cast<double>(p.cp);
    if (cpd >= ginf) {  // infeasible inside the box: every coordinate that can move goes to its bound
        if (threadIdx.x == 0) *lam_out = INFINITY, *sgn_out = p.s, *nrm_out = rmax;
        return;
    }
    // T: the largest non-negative float with g(T) < c' (g(0) = 0 < c' holds, g(inf) < c' does not)
    uint32_t T = 0u;
    for (int bit = 30; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        const float tf = __uint_as_float(cand);
        double part = 0.0;
        each([&](float av, float rv) { part = fma(static_cast<double>(av), static_cast<double>(fminf(tf, rv)), part); });
        if (red.sum(part) < cpd) T = cand;
    }
    // the segment (T, next breakpoint]: g(lambda) = S + lambda A there
    const float tl = __uint_as_float(T);
    double S = 0.0, A = 0.0;
    each([&](float av, float rv) {
        if (rv <= tl)
            S = fma(static_cast<double>(av), static_cast<double>(rv), S);
        else
            A += static_cast<double>(av);
    });
    S = red.sum(S);
    A = red.sum(A);
    const float lam = A > 0.0 ? static_cast<float>((cpd - S) / A) : INFINITY;
    if (threadIdx.x == 0) *lam_out = lam, *sgn_out = p.s, *nrm_out = fminf(lam, rmax);
}

// ---- L2: mu, with g(mu) = sum_i |v_i| min(mu |v_i|, r_i) and the breakpoints t_i = ratio(|v_i|, r_i) ---------------------------------------
template <class Each>
__device__ __forceinline__ void solve_l2(Each each, const Problem &p, SampleReducer &red, float *mu_out, float *sgn_out, float *nrm_out) {
    // g(inf) = sum |v_i| r_i
    double ginf = 0.0;
    each([&](float av, float rv, float) { ginf = fma(static_cast<double>(av), static_cast<double>(rv), ginf); });
    ginf = red.sum(ginf);
    const double cpd = static_cast<double>(p.cp);
    if (cpd >= ginf) {  // infeasible inside the box: every coordinate that can move goes to its bound
        double rs = 0.0;
        each([&](float av, float rv, float) {
            if (av != 0.0f) rs = fma(static_cast<double>(rv), static_cast<double>(rv), rs);
        });
        rs = red.sum(rs);
        if (threadIdx.x == 0) *mu_out = INFINITY, *sgn_out = p.s, *nrm_out = static_cast<float>(sqrt(rs));
        return;
    }
    // g(T) = sum_{t_i <= T} |v_i| r_i + T sum_{t_i > T} v_i^2 (v_i^2 is exact in double).  T: the largest non-negative float with
    // g(T) < c'.  g(0) = 0 < c' holds; at T = +inf every coordinate is saturated and the sum is ginf, term for term, which is not below
    // c' - so T stays finite and no candidate is a NaN pattern.
    uint32_t T = 0u;
    for (int bit = 30; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        const float tf = __uint_as_float(cand);
        const double td = static_cast<double>(tf);
        double part = 0.0;
        each([&](float av, float rv, float tv) {
            const double ad = static_cast<double>(av);
            const bool sat = tv <= tf;
            part = fma(sat ? ad : ad * ad, sat ? static_cast<double>(rv) : td, part);
        });
        if (red.sum(part) < cpd) T = cand;
    }
    // the segment (T, next breakpoint]: g(mu) = S + mu A there
    const float tl = __uint_as_float(T);
    double S = 0.0, A = 0.0;
    each([&](float av, float rv, float tv) {
        const double ad = static_cast<double>(av);
        if (tv <= tl)
            S = fma(ad, static_cast<double>(rv), S);
        else
            A = fma(ad, ad, A);
    });
    S = red.sum(S);
    A = red.sum(A);
    const double mud = A > 0.0 ? (cpd - S) / A : static_cast<double>(INFINITY);
    // ||delta||_2 from the solution before its rounding to float: the emitted norm is the correctly rounded one (or its neighbour)
    double n2 = 0.0;
    each([&](float av, float rv, float) {
        const double m = av != 0.0f ? fmin(mud * static_cast<double>(av), static_cast<double>(rv)) : 0.0;  // never inf * 0
        n2 = fma(m, m, n2);
    });
    n2 = red.sum(n2);
    if (threadIdx.x == 0) *mu_out = static_cast<float>(mud), *sgn_out = p.s, *nrm_out = static_cast<float>(sqrt(n2));
}

// ---- L1: the knapsack fill by descending |v_i| ---------------------------------------------------------------------------------------------
// F(T) = sum_{a_i >= T} a_i r_i in double (the products are exact there), in the one order of ee_sample.hpp: a sum of non-negative terms in
// a fixed order is monotone in every term, so the computed F is non-increasing in T like the real one and the bit search below is sound.
// A coordinate with a_i == 0 has the room 0 and adds an exact zero wherever it is counted.
template <class Each>
__device__ __forceinline__ void solve_l1(Each each, const Problem &p, SampleReducer &red, float *theta_out, float *sgn_out, float *nrm_out, float *phi_out) {
    // F at the smallest positive float: every moving coordinate at its bound
    double full = 0.0;
    each([&](float av, float rv) { full = fma(static_cast<double>(av), static_cast<double>(rv), full); });
    full = red.sum(full);
    const double cpd = static_cast<double>(p.cp);
    if (cpd > full) {  // infeasible inside the box: every coordinate that can move goes to its bound (all |v_i| != 0 are above theta = 0)
        double rs = 0.0;
        each([&](float av, float rv) { rs += av != 0.0f ? static_cast<double>(rv) : 0.0; });
        rs = red.sum(rs);
        if (threadIdx.x == 0) *theta_out = 0.0f, *sgn_out = p.s, *nrm_out = static_cast<float>(rs), *phi_out = 1.0f;
        return;
    }
    // theta: the largest positive float with F(theta) >= c'.  F(2^-149) = full >= c' holds, so bit 0 at the latest is taken and theta > 0;
    // w is finite (sabs is), so F is 0 < c' at +inf and at every NaN pattern (no a_i >= NaN): theta stays finite.
    uint32_t T = 0u;
    for (int bit = 30; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        const float tf = __uint_as_float(cand);
        double part = 0.0;
        each([&](float av, float rv) {
            part = fma(static_cast<double>(av), av >= tf ? static_cast<double>(rv) : 0.0, part);  // an exact zero below T
        });
        if (red.sum(part) >= cpd) T = cand;
    }
    // the fill: S and N above theta (at their bounds), P and R at theta (they share what is left of c')
    const float theta = __uint_as_float(T);
    double S = 0.0, N = 0.0, P = 0.0, R = 0.0;
    each([&](float av, float rv) {
        const double ad = static_cast<double>(av), rd = static_cast<double>(rv);
        const double above = av > theta ? rd : 0.0, at = av == theta ? rd : 0.0;  // adding an exact zero changes no sum
        S = fma(ad, above, S);
        N += above;
        P = fma(ad, at, P);
        R += at;
    });
    S = red.sum(S);
    N = red.sum(N);
    P = red.sum(P);
    R = red.sum(R);
    const double phid = P > 0.0 ? fmin(fmax((cpd - S) / P, 0.0), 1.0) : 0.0;
    // ||delta||_1 from the fraction before its rounding to float: the emitted norm is rounded once
    if (threadIdx.x == 0) *theta_out = theta, *sgn_out = p.s, *nrm_out = static_cast<float>(fma(phid, R, N)), *phi_out = static_cast<float>(phid);
}

// out [3, 2B] - L1: [4, 2B] - rows head (lambda, mu or theta), sign, ||delta||, and in L1 phi
template <bool RES, bool VEC, int M>
__global__ __launch_bounds__(kSampleBlock) void proj_kernel(const float *__restrict__ x, const float *__restrict__ x0, const float *__restrict__ w,
                                                          const float *__restrict__ df, int B, int64_t D, float *__restrict__ out) {
    __shared__ double sh[2 * kSampleWaves];
    SampleReducer red{sh};
    const int64_t Q = 2 * static_cast<int64_t>(B), q = blockIdx.x;
    float *head_out = out + q, *sgn_out = out + Q + q, *nrm_out = out + 2 * Q + q, *phi_out = M == kL1 ? out + 3 * Q + q : nullptr;
    constexpr bool BRK = M == kL2;
    Problem p;
    float a[kSampleElems], r[kSampleElems];
    Breaks<BRK> t;
    // a degenerate problem moves nothing.  No hyperplane: sign 0, and step leaves the sample where it is.  On it: sign 1 and a head under
    // which no coordinate moves - lambda = mu = 0, and theta = +inf (no |v_i| is above it)
    const auto rest = [&](bool on) {
        if (threadIdx.x != 0) return;
        *head_out = M == kL1 && on ? INFINITY : 0.0f, *sgn_out = on ? 1.0f : 0.0f, *nrm_out = 0.0f;
        if (M == kL1) *phi_out = 0.0f;
    };
    if (!proj_begin<RES, VEC, BRK>(x, x0, w, df, B, D, red, p, a, r, t, rest)) return;
    const auto each = [&](auto body) { each_element<RES, VEC, BRK>(p, a, r, t, body); };
    if constexpr (M == kL2)
        solve_l2(each, p, red, head_out, sgn_out, nrm_out);
    else if constexpr (M == kL1)
        solve_l1(each, p, red, head_out, sgn_out, nrm_out, phi_out);
    else
        solve_linf(each, p, red, head_out, sgn_out, nrm_out);
}

// ---- the step ------------------------------------------------------------------------------------------------------------------------

struct StepSample {
    float l1, s1, l2, s2, alpha;
    float phi1, phi2;  // kL1 only: the fraction of its room a coordinate AT theta takes (row 3 of the [4, 2B] scalars)
};

template <int M>
__device__ __forceinline__ StepSample step_sample(const float *__restrict__ scal, int64_t B, int64_t b) {
    StepSample r;
    r.l1 = scal[b], r.l2 = scal[B + b];
    r.s1 = scal[2 * B + b], r.s2 = scal[3 * B + b];
    const float a1 = fmaxf(scal[4 * B + b], 1e-8f), a2 = fmaxf(scal[5 * B + b], 1e-8f);
    r.alpha = fminf(a1 / (a1 + a2), kAlphaMax);
    if (M == kL1) r.phi1 = scal[6 * B + b], r.phi2 = scal[7 * B + b];
    return r;
}

// L2: delta_i = -sign(v_i) min(mu |v_i|, r_i), the product rounded once; |v_i| = 0 rests, so mu = inf never meets a 0
__device__ __forceinline__ float delta_l2(float v, float p, float mu) {
    const float a = fabsf(v);
    return a != 0.0f ? -sgn(v) * tmin(mu * a, room(v, p)) : 0.0f;
}

// L1: delta_i = -sign(v_i) m_i, m_i = r_i above theta, phi r_i (one f32 product) at theta, 0 below it - and 0 where v_i is 0 or NaN (no
// comparison holds), so theta = 0 (infeasible, phi = 1) never moves a coordinate without a direction
__device__ __forceinline__ float delta_l1(float v, float p, float theta, float phi) {
    const float a = fabsf(v), r = room(v, p);
    const float m = a > theta ? r : (a == theta && a != 0.0f ? phi * r : 0.0f);
    return -sgn(v) * m;
}

template <int M>
__device__ __forceinline__ float step_op(float x, float x0, float w, const StepSample &sm) {
    if (sm.s1 == 0.0f) return x;  // a sample without a hyperplane stays where it is
    const float v1 = sm.s1 * w, v2 = sm.s2 * w;
    float d1, d2;
    if constexpr (M == kL1) {
        d1 = delta_l1(v1, x, sm.l1, sm.phi1);
        d2 = delta_l1(v2, x0, sm.l2, sm.phi2);
    } else {
        d1 = M == kL2 ? delta_l2(v1, x, sm.l1) : -sgn(v1) * fminf(sm.l1, room(v1, x));
        d2 = M == kL2 ? delta_l2(v2, x0, sm.l2) : -sgn(v2) * fminf(sm.l2, room(v2, x0));
    }
    return tclamp((x + kEta * d1) * (1.0f - sm.alpha) + (x0 + kEta * d2) * sm.alpha, 0.0f, 1.0f);
}

template <int VEC, int M>
__global__ __launch_bounds__(kBlock) void step_kernel(float *x, const float *__restrict__ x0, const float *__restrict__ w,
                                                      const float *__restrict__ scal, int64_t B, int64_t per_sample) {
    const int64_t n = B * per_sample;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t nv = VEC == 4 ? (n >> 2) : 0;
    for (int64_t v = i; v < nv; v += stride) {
        const float4 vx = reinterpret_cast<const float4 *>(x)[v];
        const float4 v0 = reinterpret_cast<const float4 *>(x0)[v];
        const float4 vw = reinterpret_cast<const float4 *>(w)[v];
        const int64_t base = v << 2;
        const int64_t b = base / per_sample;
        const float xi[4] = {vx.x, vx.y, vx.z, vx.w}, oi[4] = {v0.x, v0.y, v0.z, v0.w}, wi[4] = {vw.x, vw.y, vw.z, vw.w};
        float out[4];
        if (base - b * per_sample + 4 <= per_sample) {  // the four elements belong to one sample
            const StepSample sm = step_sample<M>(scal, B, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = step_op<M>(xi[k], oi[k], wi[k], sm);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) out[k] = step_op<M>(xi[k], oi[k], wi[k], step_sample<M>(scal, B, (base + k) / per_sample));  // base + k < n
        }
        reinterpret_cast<float4 *>(x)[v] = make_float4(out[0], out[1], out[2], out[3]);
    }
    for (int64_t e = (nv << 2) + i; e < n; e += stride) x[e] = step_op<M>(x[e], x0[e], w[e], step_sample<M>(scal, B, e / per_sample));
}

// ---- the check after the second forward ------------------------------------------------------------------------------------------------
// ||x - x0||_inf of the sample at `off`; every thread gets it
template <int VEC>
__device__ __forceinline__ float commit_norm_linf(const float *x, const float *x0, int64_t off, int64_t per_sample) {
    __shared__ float sh_max[kSampleWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    float m = 0.0f;
    if (VEC == 4) {  // per_sample % 4 == 0 and 16-byte bases: a sample is a whole number of aligned vectors
        const float4 *vx = reinterpret_cast<const float4 *>(x + off), *v0 = reinterpret_cast<const float4 *>(x0 + off);
        for (int64_t v = threadIdx.x; v < (per_sample >> 2); v += kSampleBlock) {
            const float4 p = vx[v], o = v0[v];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(p.x - o.x), fabsf(p.y - o.y)), fmaxf(fabsf(p.z - o.z), fabsf(p.w - o.w))));
        }
    } else {
        for (int64_t k = threadIdx.x; k < per_sample; k += kSampleBlock) m = fmaxf(m, fabsf(x[off + k] - x0[off + k]));
    }
    m = wave_max(m);
    if (lane == 0) sh_max[wave] = m;
    __syncthreads();
    m = sh_max[0];
#pragma unroll
    for (int i = 1; i < kSampleWaves; ++i) m = fmaxf(m, sh_max[i]);
    return m;
}

// ||x - x0||_2 of the sample at `off` - the squares of the f32 differences summed in double in the order of the projection (ee_sample.hpp's,
// whatever the access width), so vector and element-wise calls return the same bits
template <bool VEC>
__device__ __forceinline__ float commit_norm_l2(const float *x, const float *x0, int64_t off, int64_t per_sample) {
    __shared__ double sh_sum[kSampleWaves];  // one reduction: it uses the first half of the reducer's buffer only
    SampleReducer red{sh_sum};
    double sq = 0.0;
    for (int64_t e = static_cast<int64_t>(threadIdx.x) * 4; e < per_sample; e += kSampleBlock * 4) {
        float pv[4], ov[4];
        load4<VEC>(x + off, e, per_sample, pv);
        load4<VEC>(x0 + off, e, per_sample, ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = static_cast<double>(pv[j] - ov[j]);
            sq = fma(d, d, sq);
        }
    }
    return static_cast<float>(sqrt(red.sum(sq)));
}

// ||x - x0||_1 of the sample at `off`: the |f32 differences| summed in double in the order of commit_norm_l2, rounded to float once
template <bool VEC>
__device__ __forceinline__ float commit_norm_l1(const float *x, const float *x0, int64_t off, int64_t per_sample) {
    __shared__ double sh_sum[kSampleWaves];  // one reduction: it uses the first half of the reducer's buffer only
    SampleReducer red{sh_sum};
    double sa = 0.0;
    for (int64_t e = static_cast<int64_t>(threadIdx.x) * 4; e < per_sample; e += kSampleBlock * 4) {
        float pv[4], ov[4];
        load4<VEC>(x + off, e, per_sample, pv);
        load4<VEC>(x0 + off, e, per_sample, ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) sa += static_cast<double>(fabsf(pv[j] - ov[j]));
    }
    return static_cast<float>(red.sum(sa));
}

// M picks the distance: ||x - x0||_inf, ||x - x0||_2 or ||x - x0||_1.  Everything else is one code.
template <int VEC, int M>
__global__ __launch_bounds__(kSampleBlock) void commit_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels, int K, float *x,
                                                              const float *__restrict__ x0, float *adv, float *res, int *__restrict__ pred,
                                                              int *__restrict__ flags, int *counter, int64_t per_sample) {
    __shared__ int sh_first, sh_nan;
    const int b = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (b == 0 && threadIdx.x == 0) counter[0] = counter[0] + 1;  // nobody reads the counter in this launch
    const float best = res[b];  // read by every thread before the barrier below, written by thread 0 after it
    if (wave == 0) {
        bool nan;
        const int first = row_first(logits + static_cast<size_t>(b) * K, K, lane, nan);
        if (lane == 0) sh_first = first, sh_nan = nan ? 1 : 0;
    }
    const int64_t off = static_cast<int64_t>(b) * per_sample;
    // the distance; the barrier inside also publishes sh_first / sh_nan
    float m;
    if constexpr (M == kL2)
        m = commit_norm_l2<VEC == 4>(x, x0, off, per_sample);
    else if constexpr (M == kL1)
        m = commit_norm_l1<VEC == 4>(x, x0, off, per_sample);
    else
        m = commit_norm_linf<VEC>(x, x0, off, per_sample);
    const int64_t y = labels[b];
    const int first = sh_first;
    const bool is_adv = !sh_nan && y >= 0 && y < K && first != y;  // a row with a NaN logit is never adversarial
    const bool improve = is_adv && m < best;
    if (threadIdx.x == 0) {
        pred[b] = first;
        flags[b] = (is_adv ? EE_FAB_ADV : 0) | (improve ? EE_FAB_IMPROVED : 0);
        if (improve) res[b] = m;
    }
    if (!is_adv) return;
    if (VEC == 4) {
        float4 *vx = reinterpret_cast<float4 *>(x + off), *va = reinterpret_cast<float4 *>(adv + off);
        const float4 *v0 = reinterpret_cast<const float4 *>(x0 + off);
        for (int64_t v = threadIdx.x; v < (per_sample >> 2); v += kSampleBlock) {
            const float4 p = vx[v], o = v0[v];
            if (improve) va[v] = p;
            vx[v] = make_float4(o.x + kBeta * (p.x - o.x), o.y + kBeta * (p.y - o.y), o.z + kBeta * (p.z - o.z), o.w + kBeta * (p.w - o.w));
        }
    } else {
        for (int64_t k = threadIdx.x; k < per_sample; k += kSampleBlock) {
            const float p = x[off + k], o = x0[off + k];
            if (improve) adv[off + k] = p;
            x[off + k] = o + kBeta * (p - o);
        }
    }
}

// ---- untargeted FAB: the running arg-min over the classes -------------------------------------------------------------------------------
// One launch per class k, after that class's backward pass: n_k = the dual norm of the row g[b] (M = kLinf: sum |g_i|, kL2: sqrt(sum g_i^2),
// kL1: max |g_i|; the sums in double in the one order of ee_sample.hpp, rounded to float once), dist = |df_k| / (1e-12 + n_k) in float, and -
// where dist is strictly below best[b] - the sample takes the class: best, best_k, df, and the row copied into w.  Strict `<` over ascending
// k keeps the lowest class among equal distances.  `first` (class 0's launch) stands in for the reset: the old best / best_k / df are not read
// and are always written.  A sample belongs to one workgroup; best[b] is read by every thread before the reduction's barrier and written
// by thread 0 after it.  One streaming pass: a row is read once for the norm and, on improvement, once more (from L2) for the copy - there
// is nothing to keep resident across passes, so no resident / streaming pair.
template <bool VEC, int M>
__global__ __launch_bounds__(kSampleBlock) void select_kernel(const float *__restrict__ g, const float *__restrict__ logits,
                                                              const int64_t *__restrict__ labels, int k, int K, int first, int64_t D,
                                                              float *best, int *best_k, float *__restrict__ w, float *df) {
    __shared__ double sh[2 * kSampleWaves];
    SampleReducer red{sh};
    const int b = blockIdx.x;
    const float *gr = g + static_cast<int64_t>(b) * D;
    const int groups = groups_of(D);
    const float cur = first ? INFINITY : best[b];
    double acc = 0.0;
    for (int q = 0; q < groups; ++q) {
        float gv[4];
        load4<VEC>(gr, group_element(q), D, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = fabsf(gv[j]);
            if constexpr (M == kL2)
                acc = fma(static_cast<double>(a), static_cast<double>(a), acc);
            else if constexpr (M == kL1)
                acc = a != a ? static_cast<double>(INFINITY) : fmax(acc, static_cast<double>(a));  // a NaN makes the norm not finite, as in a sum
            else
                acc += static_cast<double>(a);
        }
    }
    float n;
    if constexpr (M == kL2)
        n = static_cast<float>(sqrt(red.sum(acc)));
    else if constexpr (M == kL1)
        n = static_cast<float>(red.max(acc));  // the largest |g_i|, a float: exact
    else
        n = static_cast<float>(red.sum(acc));
    const int64_t y = labels[b];
    const bool valid = y >= 0 && y < K;  // a label outside the row is never dereferenced
    const float *z = logits + static_cast<size_t>(b) * K;
    const float d = valid ? z[k] - z[y] : NAN;
    const bool live = valid && y != k && isfinite(d) && isfinite(n) && n != 0.0f;
    const float dist = fabsf(d) / (1e-12f + n);
    const bool take = live && dist < cur;  // uniform over the workgroup
    if (threadIdx.x == 0) {
        if (take)
            best[b] = dist, best_k[b] = k, df[b] = d;
        else if (first)
            best[b] = INFINITY, best_k[b] = -1, df[b] = 0.0f;
    }
    if (!take) return;
    float *wr = w + static_cast<int64_t>(b) * D;
    for (int q = 0; q < groups; ++q) {
        const int64_t e = group_element(q);
        float gv[4];
        load4<VEC>(gr, e, D, gv);
        store4<VEC>(wr, e, D, gv);
    }
}

// ---- the random start of a restart ---------------------------------------------------------------------------------
// x = clamp(x0 + ((m t) / n) / 2, 0, 1) with m = min(res[b], eps), t a draw of D elements and n its norm in the threat model's own metric
// (M = kLinf: max |t_i|, kL2: sqrt(sum t_i^2), kL1: sum |t_i|; the sums in double in the one order of ee_sample.hpp, rounded to float once).
// DRAW (start_draw4 of ee_sample.hpp, under kStreamFabStart): t comes from Philox, one call per group of four elements under the counter (b << 32) | (e >> 2) - a row's draw depends on (seed, b,
// element) alone - uniform on [-1, 1) for Linf, standard normal otherwise; else t is the row of `noise`.  RES keeps t in registers between
// the norm pass and the write pass, the streaming path reads or draws it again.  A row whose n is 0 or not finite is written as x0.  The
// launch reads res and writes x: no scalar crosses workgroups.
template <bool RES, bool VEC, int M, bool DRAW>
__global__ __launch_bounds__(kSampleBlock) void start_kernel(float *__restrict__ x, const float *__restrict__ x0, const float *__restrict__ res,
                                                           const float *__restrict__ noise, int64_t D, float eps, uint64_t seed) {
    __shared__ double sh[2 * kSampleWaves];
    SampleReducer red{sh};
    const int b = blockIdx.x;
    const int64_t off = static_cast<int64_t>(b) * D;
    const float *x0r = x0 + off, *nr = DRAW ? nullptr : noise + off;
    float *xr = x + off;
    const Philox ph(seed);
    const int groups = groups_of(D);

    // pass 1: the norm of the draw; the resident path keeps the draw in keep[]
    float keep[kSampleElems];
    double acc = 0.0;
    auto first = [&](int g) {
        float t[4];
        start_draw4<kStreamFabStart, M == kLinf, DRAW, VEC>(ph, nr, b, group_element(g), D, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = fabsf(t[j]);
            if constexpr (M == kL2)
                acc = fma(static_cast<double>(a), static_cast<double>(a), acc);
            else if constexpr (M == kL1)
                acc += static_cast<double>(a);
            else
                acc = a != a ? static_cast<double>(INFINITY) : fmax(acc, static_cast<double>(a));  // a NaN makes the norm not finite, as in a sum
            if (RES) keep[g * 4 + j] = t[j];
        }
    };
    if (RES) {
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) first(g);
    } else {
        for (int g = 0; g < groups; ++g) first(g);
    }
    float n;
    if constexpr (M == kL2)
        n = static_cast<float>(sqrt(red.sum(acc)));
    else if constexpr (M == kL1)
        n = static_cast<float>(red.sum(acc));
    else
        n = static_cast<float>(red.max(acc));  // the largest |t_i|, a float: exact
    const float m = fminf(res[b], eps);
    const bool live = isfinite(n) && n != 0.0f;  // uniform over the workgroup

    // pass 2: the point, every operation rounded once
    auto second = [&](int g) {
        const int64_t e = group_element(g);
        float t[4], ov[4], out[4];
        if (RES) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = keep[g * 4 + j];
        } else {
            start_draw4<kStreamFabStart, M == kLinf, DRAW, VEC>(ph, nr, b, e, D, t);
        }
        load4<VEC>(x0r, e, D, ov);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = live ? tclamp(ov[j] + ((m * t[j]) / n) * 0.5f, 0.0f, 1.0f) : ov[j];
        store4<VEC>(xr, e, D, out);
    };
    if (RES) {
#pragma unroll
        for (int g = 0; g < kSampleVecs; ++g) second(g);
    } else {
        for (int g = 0; g < groups; ++g) second(g);
    }
}

bool bad_shape(int64_t B, int64_t per_sample) {
    return B < 0 || per_sample < 0 || B > INT32_MAX / 2 || per_sample > INT32_MAX || (per_sample > 0 && B > INT64_MAX / per_sample);
}

// ---- the launches that differ between Linf, L2 and L1 in one template argument ------------------------------------------------------------
template <int M>
int launch_proj(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path, float *out,
                void *stream) {
    if (bad_shape(B, per_sample) || per_sample < 1) return EE_ERR_SHAPE;
    bool res;
    if (const int rc = sample_path(path, per_sample, &res)) return rc;
    if (B == 0) return EE_OK;
    if (!x || !x0 || !w || !df || !out) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(x0) || !aligned4(w) || !aligned4(df) || !aligned4(out)) return EE_ERR_ALIGN;
    const dim3 grid(static_cast<unsigned>(2 * B)), block(kSampleBlock);
    const int nb = static_cast<int>(B);
    ProfScope prof(EE_K_FAB_PROJ, as_stream(stream));
    sample_launch(res, sample_vec(per_sample, x, x0, w), [&](auto RES, auto VEC) {
        EE_LAUNCH((proj_kernel<RES, VEC, M>), grid, block, 0, as_stream(stream), x, x0, w, df, nb, per_sample, out);
    });
    return launch_status();
}

template <int M>
int launch_step(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream) {
    if (bad_shape(B, per_sample)) return EE_ERR_SHAPE;
    const int64_t n = B * per_sample;
    if (n == 0) return EE_OK;
    if (!x || !x0 || !w || !scal) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(x0) || !aligned4(w) || !aligned4(scal)) return EE_ERR_ALIGN;
    const bool vec = aligned16(x) && aligned16(x0) && aligned16(w);
    const unsigned blocks = grid_for(vec ? (n + 3) / 4 : n);
    ProfScope prof(EE_K_FAB_STEP, as_stream(stream));
    if (vec)
        EE_LAUNCH((step_kernel<4, M>), dim3(blocks), dim3(kBlock), 0, as_stream(stream), x, x0, w, scal, B, per_sample);
    else
        EE_LAUNCH((step_kernel<1, M>), dim3(blocks), dim3(kBlock), 0, as_stream(stream), x, x0, w, scal, B, per_sample);
    return launch_status();
}

template <int M>
int launch_commit(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res, int *pred,
                  int *flags, int *counter, int64_t per_sample, void *stream) {
    if (B < 0 || K < 2 || K > 65536 || bad_shape(B, per_sample)) return EE_ERR_SHAPE;
    if (B == 0 || per_sample == 0) return EE_OK;  // an empty batch is no attack: nothing is launched, the counter stays
    if (!logits || !labels || !x || !x0 || !adv || !res || !pred || !flags || !counter) return EE_ERR_NULL;
    if (!aligned4(logits) || !aligned4(x) || !aligned4(x0) || !aligned4(adv) || !aligned4(res) || !aligned4(pred) || !aligned4(flags) ||
        !aligned4(counter) || (reinterpret_cast<uintptr_t>(labels) & 7u))
        return EE_ERR_ALIGN;
    const dim3 grid(static_cast<unsigned>(B)), block(kSampleBlock);
    ProfScope prof(EE_K_FAB_COMMIT, as_stream(stream));
    if (sample_vec(per_sample, x, x0, adv))
        EE_LAUNCH((commit_kernel<4, M>), grid, block, 0, as_stream(stream), logits, labels, K, x, x0, adv, res, pred, flags, counter, per_sample);
    else
        EE_LAUNCH((commit_kernel<1, M>), grid, block, 0, as_stream(stream), logits, labels, K, x, x0, adv, res, pred, flags, counter, per_sample);
    return launch_status();
}

template <int M>
int launch_select(const float *g, const float *logits, const int64_t *labels, int k, int K, int first, int64_t B, int64_t per_sample, float *best,
                  int *best_k, float *w, float *df, void *stream) {
    const dim3 grid(static_cast<unsigned>(B)), block(kSampleBlock);
    if (sample_vec(per_sample, g, w))
        EE_LAUNCH((select_kernel<true, M>), grid, block, 0, as_stream(stream), g, logits, labels, k, K, first, per_sample, best, best_k, w, df);
    else
        EE_LAUNCH((select_kernel<false, M>), grid, block, 0, as_stream(stream), g, logits, labels, k, K, first, per_sample, best, best_k, w, df);
    return launch_status();
}

template <int M>
int launch_start(float *x, const float *x0, const float *res, const float *noise, int64_t B, int64_t per_sample, float eps, uint64_t seed,
                 bool resident, void *stream) {
    const dim3 grid(static_cast<unsigned>(B)), block(kSampleBlock);
    sample_launch(resident, sample_vec(per_sample, x, x0, noise), [&](auto RES, auto VEC) {  // a null noise counts as aligned: it is not read
        if (noise)
            EE_LAUNCH((start_kernel<RES, VEC, M, false>), grid, block, 0, as_stream(stream), x, x0, res, noise, per_sample, eps, seed);
        else
            EE_LAUNCH((start_kernel<RES, VEC, M, true>), grid, block, 0, as_stream(stream), x, x0, res, noise, per_sample, eps, seed);
    });
    return launch_status();
}

}  // namespace

EE_API int ee_fab_start_f32(float *x, const float *x0, const float *res, const float *noise, int64_t B, int64_t per_sample, float eps, int metric,
                            uint64_t seed, int path, void *stream) {
    if (bad_shape(B, per_sample) || per_sample < 1 || metric < kLinf || metric > kL1 || !(eps >= 0.0f)) return EE_ERR_SHAPE;
    bool resident;
    if (const int rc = sample_path(path, per_sample, &resident)) return rc;
    if (B == 0) return EE_OK;
    if (!x || !x0 || !res) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(x0) || !aligned4(res) || !aligned4(noise)) return EE_ERR_ALIGN;
    ProfScope prof(EE_K_FAB_STEP, as_stream(stream));
    if (metric == kL2) return launch_start<kL2>(x, x0, res, noise, B, per_sample, eps, seed, resident, stream);
    if (metric == kL1) return launch_start<kL1>(x, x0, res, noise, B, per_sample, eps, seed, resident, stream);
    return launch_start<kLinf>(x, x0, res, noise, B, per_sample, eps, seed, resident, stream);
}

EE_API int ee_fab_select_f32(const float *g, const float *logits, const int64_t *labels, int k, int metric, int first, int64_t B, int K,
                             int64_t per_sample, float *best, int *best_k, float *w, float *df, void *stream) {
    if (bad_shape(B, per_sample) || per_sample < 1 || K < 2 || K > 65536 || k < 0 || k >= K || metric < kLinf || metric > kL1) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!g || !logits || !labels || !best || !best_k || !w || !df) return EE_ERR_NULL;
    if (!aligned4(g) || !aligned4(logits) || !aligned4(best) || !aligned4(best_k) || !aligned4(w) || !aligned4(df) ||
        (reinterpret_cast<uintptr_t>(labels) & 7u))
        return EE_ERR_ALIGN;
    ProfScope prof(EE_K_FAB_DIFF, as_stream(stream));
    if (metric == kL2) return launch_select<kL2>(g, logits, labels, k, K, first != 0, B, per_sample, best, best_k, w, df, stream);
    if (metric == kL1) return launch_select<kL1>(g, logits, labels, k, K, first != 0, B, per_sample, best, best_k, w, df, stream);
    return launch_select<kLinf>(g, logits, labels, k, K, first != 0, B, per_sample, best, best_k, w, df, stream);
}

EE_API int ee_fab_diff_f32(const float *logits, const int64_t *labels, const int64_t *targets, int B, int K, float *df, float *dlogits, int *pred,
                           void *stream) {
    if (B < 0 || K < 2 || K > 65536) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!logits || !labels || !targets || !df || !dlogits || !pred) return EE_ERR_NULL;
    if (!aligned4(logits) || !aligned4(df) || !aligned4(dlogits) || !aligned4(pred) || (reinterpret_cast<uintptr_t>(labels) & 7u) ||
        (reinterpret_cast<uintptr_t>(targets) & 7u))
        return EE_ERR_ALIGN;
    ProfScope prof(EE_K_FAB_DIFF, as_stream(stream));
    EE_LAUNCH(diff_kernel, dim3(row_grid(B)), dim3(kBlock), 0, as_stream(stream), logits, labels,
              targets, B, K, df, dlogits, pred);
    return launch_status();
}

EE_API int ee_fab_proj_linf_f32(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path,
                                float *out, void *stream) {
    return launch_proj<kLinf>(x, x0, w, df, B, per_sample, path, out, stream);
}

EE_API int ee_fab_proj_l2_f32(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path,
                              float *out, void *stream) {
    return launch_proj<kL2>(x, x0, w, df, B, per_sample, path, out, stream);
}

EE_API int ee_fab_step_f32(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream) {
    return launch_step<kLinf>(x, x0, w, scal, B, per_sample, stream);
}

EE_API int ee_fab_step_l2_f32(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream) {
    return launch_step<kL2>(x, x0, w, scal, B, per_sample, stream);
}

EE_API int ee_fab_commit_f32(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res, int *pred,
                             int *flags, int *counter, int64_t per_sample, void *stream) {
    return launch_commit<kLinf>(logits, labels, B, K, x, x0, adv, res, pred, flags, counter, per_sample, stream);
}

EE_API int ee_fab_commit_l2_f32(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res,
                                int *pred, int *flags, int *counter, int64_t per_sample, void *stream) {
    return launch_commit<kL2>(logits, labels, B, K, x, x0, adv, res, pred, flags, counter, per_sample, stream);
}

EE_API int ee_fab_proj_l1_f32(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path,
                              float *out, void *stream) {
    return launch_proj<kL1>(x, x0, w, df, B, per_sample, path, out, stream);
}

EE_API int ee_fab_step_l1_f32(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream) {
    return launch_step<kL1>(x, x0, w, scal, B, per_sample, stream);
}

EE_API int ee_fab_commit_l1_f32(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res,
                                int *pred, int *flags, int *counter, int64_t per_sample, void *stream) {
    return launch_commit<kL1>(logits, labels, B, K, x, x0, adv, res, pred, flags, counter, per_sample, stream);
}
