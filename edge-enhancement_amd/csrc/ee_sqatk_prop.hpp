// ee_sqatk_prop.hpp - what the L2 and the L1 form of the Square attack (ee_sqatk_l2.hip, ee_sqatk_l1.hip; DESIGN.md sections 18 and 21)
// share beyond ee_sqatk.hpp: what a launch knows of one element, the reducer that takes all sums of a round at once, the tiled start
// pattern, and the step launch up to the rescaled window 1 - prologue, commit, draws, rounds 1 and 2 - as one body (propose_window) over a
// norm policy.  One definition each, so the pattern, the windows and the window-1 update of an L1 run are those of an L2 run by
// construction: the two kernels run the same text and differ in the policy and in what follows the body.
#pragma once

#include "ee_sample.hpp"
#include "ee_sqatk.hpp"

namespace ee {

constexpr int kMaxC = 32;                            // one sign bit per channel
constexpr float kTiny = 1e-12f;

// bits of Info::f
constexpr uint32_t kIn1 = 1u, kIn2 = 2u;

struct Geo {
    int C, H, W, HW;
    int64_t D;
};

// what a launch knows of one element: f = kIn1 | kIn2 | channel << 8, idx = its place in the eta table (window 1 / a tile only)
struct Info {
    uint32_t f;
    int idx;
};

__device__ __forceinline__ int channel_of(const Info &i) { return static_cast<int>(i.f >> 8); }

// the sums of one round: put() every slot, then sums() - two barriers a round, whatever the number of slots
struct Reducer {
    double *part;  // [2 + kMaxC][kSampleWaves]
    __device__ __forceinline__ void put(int slot, double v) {
        v = wave_sum(v);
        if ((threadIdx.x & (kWave - 1)) == 0) part[slot * kSampleWaves + (threadIdx.x >> 6)] = v;
    }
    // out[k] = fin(the sum of slot k's partials in index order), k < n; also stored to global[row(k) * B + b]
    template <class Row, class Fin>
    __device__ __forceinline__ void sums(int n, float *out, float *__restrict__ global, int64_t B, int64_t b, Row row, Fin fin) {
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < n) {
            const double *p = part + threadIdx.x * kSampleWaves;
            double r = p[0];
#pragma unroll
            for (int i = 1; i < kSampleWaves; ++i) r += p[i];
            const float v = fin(r);
            out[threadIdx.x] = v;
            if (global) global[static_cast<int64_t>(row(static_cast<int>(threadIdx.x))) * B + b] = v;
        }
        __syncthreads();
    }
};

// Info of the four elements from e on, `one(c, h, w)` giving an element's; elements at or past D get {0, 0}
template <class F>
__device__ __forceinline__ void infos4(int64_t e, const Geo &g, Info (&o)[4], F one) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = Info{0u, 0};
    if (e >= g.D) return;
    const int r = static_cast<int>(e);
    int c = r / g.HW;
    const int rem = r - c * g.HW;
    int h = rem / g.W, w = rem - h * g.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (e + j < g.D) o[j] = one(c, h, w);
        if (++w == g.W) {
            w = 0;
            if (++h == g.H) h = 0, ++c;
        }
    }
}

// ---- start ---------------------------------------------------------------------------------------------------------------------------
// the tiled pattern d of sample `id`'s start, as both start kernels read it
struct Tiling {
    Philox ph;
    int s0, nh, nw, oh, ow;
    int64_t id;
    const float *eta;
    __device__ __forceinline__ Tiling(const int64_t *seed, const float *eta0, int s, int H, int W, int64_t b)
        : ph(static_cast<uint64_t>(seed[0])), s0(s), nh(H / s), nw(W / s), oh((H - nh * s) / 2), ow((W - nw * s) / 2), id(b), eta(eta0) {}
    // d of the four elements from e on; 0 at or past D (an element's d travels in Info::idx as its bits)
    __device__ __forceinline__ void d4(int64_t e, const Geo &geo, float (&dv)[4]) const {
        Info in[4];
        infos4(e, geo, in, [&](int c, int h, int w) { return Info{0u, __float_as_int(value(c, h, w))}; });
#pragma unroll
        for (int j = 0; j < 4; ++j) dv[j] = __int_as_float(in[j].idx);
    }
    // d of element (c, h, w): +-eta0[r][q], transposed by the tile's coin; 0 outside the tiling
    __device__ __forceinline__ float value(int c, int h, int w) const {
        const int th = h - oh, tw = w - ow;
        if (th < 0 || tw < 0) return 0.0f;
        const int a = th / s0, bt = tw / s0;
        if (a >= nh || bt >= nw) return 0.0f;
        const int r = th - a * s0, q = tw - bt * s0;
        const uint4 d = ph((static_cast<uint64_t>(id) << 32) | static_cast<uint32_t>(a * nw + bt), kStreamTile);
        const float e = eta[(d.y & 1u) ? q * s0 + r : r * s0 + q];
        return ((d.x >> c) & 1u) ? e : -e;
    }
};

// ---- proposal ------------------------------------------------------------------------------------------------------------------------
// the element-wise lines of a proposal up to the rescaled window 1; the scalars are filled in as the norms become known (n_w, n_new live
// in LDS).  What a threat model does with the result - and which norm n_w, n_new and scale are - is its own file's.
struct Proposal {
    int s, vh, vw, vh2, vw2;
    uint32_t signs;
    bool transpose;
    const float *eta;
    const float *n_w, *n_new;
    float scale;

    __device__ __forceinline__ Info info(int c, int h, int w) const {
        Info r{static_cast<uint32_t>(c) << 8, 0};
        const int a = h - vh, q = w - vw;
        if (a >= 0 && a < s && q >= 0 && q < s) r.f |= kIn1, r.idx = transpose ? q * s + a : a * s + q;
        if (h >= vh2 && h < vh2 + s && w >= vw2 && w < vw2 + s) r.f |= kIn2;
        return r;
    }
    // delta -> new on window 1, 0 on the rest of window 2, delta elsewhere
    __device__ __forceinline__ float stage1(float delta, const Info &i) const {
        if (i.f & kIn1) {
            const int c = channel_of(i);
            const float e = eta[i.idx];
            return (((signs >> c) & 1u) ? e : -e) + delta / (kTiny + n_w[c]);
        }
        return (i.f & kIn2) ? 0.0f : delta;
    }
    // new -> new / (tiny + n_new) * scale on window 1
    __device__ __forceinline__ float stage2(float v, const Info &i) const {
        return (i.f & kIn1) ? v / (kTiny + n_new[channel_of(i)]) * scale : v;
    }
};

__device__ __forceinline__ bool any_in1(const Info (&in)[4], int c) {
    bool r = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= (in[j].f & kIn1) && channel_of(in[j]) == c;
    return r;
}

// ---- the step launch up to the rescaled window ----------------------------------------------------------------------------------------
// what ee_sqatk_step_l2_f32 and ee_sqatk_step_l1_f32 both pass to their kernel
struct StepArgs {
    float *x_best, *x_new;
    const float *x0;
    const int *flags;
    const float *margin_min;
    const int *counter, *sizes, *eta_off;
    const float *eta;
    int n_sizes;
    const int64_t *seed;
    float *norms;
    int64_t B;
    int C, H, W;
    float eps;
};

// the streaming path after round 1: (x0, delta, info) of this thread's k-th group handed to `body`, skipped when `want` says the pass
// has no use for it
template <bool VEC>
struct Stream {
    const Proposal *p;
    Geo geo;
    const float *br, *cr;
    template <class Want, class Body>
    __device__ __forceinline__ void operator()(int k, Want want, Body body) const {
        const int64_t e = group_element(k);
        Info in[4];
        infos4(e, geo, in, [&](int c, int h, int w) { return p->info(c, h, w); });
        if (!want(in)) return;
        float xv[4], cv[4], dv[4];
        load4<VEC>(br, e, geo.D, xv);
        load4<VEC>(cr, e, geo.D, cv);
#pragma unroll
        for (int j = 0; j < 4; ++j) dv[j] = xv[j] - cv[j];
        body(e, cv, dv, in);
    }
};

// One sample's step up to p.scale: the decision, the zeroed rows of a sample that proposes nothing, the commit, the two window draws, and
// rounds 1 ({n_img, n_un, n_w}) and 2 ({n_new}), two barriers each.  The norm N gives
//     term(float) -> double    what a norm sums              fin(double) -> float    the norm of a sum
//     kHead                    rows of `norms` ahead of n_w[0]: n_img, n_un (and n_d in L2); n_new follows n_w, kHead + 2C rows in all
//     scale(eps, n_img, n_un, C)
// sn1 [2 + kMaxC] and sn2 [kMaxC] are LDS.  false: the sample makes no proposal and the launch is done with it.  true: p is filled, x_best
// holds the committed point, `stream` serves the passes that follow, and on the resident path rc = x0, ri = what is known of each
// element, rv = new on window 1 (stage1 applied) - on the streaming path the three are untouched.
template <class N, bool RES, bool VEC>
__device__ __forceinline__ bool propose_window(const StepArgs &a, Reducer &red, float *sn1, float *sn2, Proposal &p, Stream<VEC> &stream,
                                               float (&rc)[kSampleElems], float (&rv)[kSampleElems], Info (&ri)[kSampleElems]) {
    const int C = a.C, H = a.H, W = a.W;
    const Geo geo{C, H, W, H * W, static_cast<int64_t>(C) * H * W};
    const int64_t b = blockIdx.x, B = a.B, D = geo.D;
    const int it = a.counter[0];
    int s = (it >= 0 && it < a.n_sizes) ? a.sizes[it] : 0;  // 0: no proposal in this launch (commit only)
    if (s < 1 || s > H || s > W) s = 0;                     // a size the window arithmetic cannot take is no proposal either
    const int off = s ? a.eta_off[it] : 0;
    if (off < 0) s = 0;
    const bool commit = a.flags[b] != 0, propose = s > 0 && !(a.margin_min[b] <= 0.0f);  // uniform over the workgroup
    if (!propose && static_cast<int>(threadIdx.x) < N::kHead + 2 * C) a.norms[static_cast<int64_t>(threadIdx.x) * B + b] = 0.0f;
    if (!commit && !propose) return false;
    const float *cr = a.x0 + b * D;
    float *br = a.x_best + b * D, *nr = a.x_new + b * D;
    const int groups = groups_of(D);
    if (!propose) {  // the commit alone
        for (int k = 0; k < groups; ++k) {
            float v[4];
            load4<VEC>(nr, group_element(k), D, v);
            store4<VEC>(br, group_element(k), D, v);
        }
        return false;
    }
    const Philox ph(static_cast<uint64_t>(a.seed[0]));
    const WindowDraw w1 = draw_window(ph, it, b, s, H, W, kStreamWindow), w2 = draw_window(ph, it, b, s, H, W, kStreamWindow2);
    p.s = s, p.vh = w1.vh, p.vw = w1.vw, p.vh2 = w2.vh, p.vw2 = w2.vw, p.signs = w1.z, p.transpose = (w1.w & 1u) != 0;
    p.eta = a.eta + off, p.n_w = sn1 + 2, p.n_new = sn2, p.scale = 0.0f;
    stream = Stream<VEC>{&p, geo, br, cr};

    // round 1: n_img, n_un over the whole sample - the pass that commits, and that takes the sample into registers on the resident path
    double a_img = 0.0, a_un = 0.0;
    const auto first = [&](int64_t e, float (&cv)[4], float (&dv)[4], Info (&in)[4]) {
        float xv[4];
        load4<VEC>(commit ? nr : br, e, D, xv);
        if (commit) store4<VEC>(br, e, D, xv);
        load4<VEC>(cr, e, D, cv);
        infos4(e, geo, in, [&](int c, int h, int w) { return p.info(c, h, w); });
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dv[j] = xv[j] - cv[j];
            const double q = N::term(dv[j]);
            a_img += q;
            a_un += (in[j].f & (kIn1 | kIn2)) ? q : 0.0;
        }
    };
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleVecs; ++k) {
            float cv[4], dv[4];
            Info in[4];
            first(group_element(k), cv, dv, in);
#pragma unroll
            for (int j = 0; j < 4; ++j) rc[k * 4 + j] = cv[j], rv[k * 4 + j] = dv[j], ri[k * 4 + j] = in[j];
        }
    } else {
        for (int k = 0; k < groups; ++k) {
            float cv[4], dv[4];
            Info in[4];
            first(group_element(k), cv, dv, in);
        }
    }
    red.put(0, a_img);
    red.put(1, a_un);
    // the sum of the terms over window 1 of channel c, put into `slot`: of rv on the resident path, of at(delta, info) on the streaming one
    const auto window1 = [&](int slot, int c, auto at) {
        double acc = 0.0;
        if (RES) {
#pragma unroll
            for (int k = 0; k < kSampleElems; ++k) acc += ((ri[k].f & kIn1) && channel_of(ri[k]) == c) ? N::term(rv[k]) : 0.0;
        } else {
            for (int k = 0; k < groups; ++k)
                stream(k, [&](const Info(&in)[4]) { return any_in1(in, c); },
                       [&](int64_t, const float(&)[4], const float(&dv)[4], const Info(&in)[4]) {
#pragma unroll
                           for (int j = 0; j < 4; ++j) acc += ((in[j].f & kIn1) && channel_of(in[j]) == c) ? N::term(at(dv[j], in[j])) : 0.0;
                       });
        }
        red.put(slot, acc);
    };
    const auto fin = [](double r) { return N::fin(r); };
    for (int c = 0; c < C; ++c) window1(2 + c, c, [](float v, const Info &) { return v; });
    red.sums(2 + C, sn1, a.norms, B, b, [](int k) { return k < 2 ? k : N::kHead - 2 + k; }, fin);
    p.scale = N::scale(a.eps, sn1[0], sn1[1], C);

    // round 2: n_new[c]
    if (RES) {
#pragma unroll
        for (int k = 0; k < kSampleElems; ++k) rv[k] = p.stage1(rv[k], ri[k]);
    }
    for (int c = 0; c < C; ++c) window1(c, c, [&](float v, const Info &i) { return p.stage1(v, i); });
    red.sums(C, sn2, a.norms, B, b, [C](int k) { return N::kHead + C + k; }, fin);
    return true;
}

}  // namespace ee
