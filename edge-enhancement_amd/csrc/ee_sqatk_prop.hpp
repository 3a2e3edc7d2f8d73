// ee_sqatk_prop.hpp - what the L2 and the L1 form of the Square attack (ee_sqatk_l2.hip, ee_sqatk_l1.hip; DESIGN.md sections 18 and 21)
// share beyond ee_sqatk.hpp: what a launch knows of one element, the tiled start pattern, the element-wise lines of a proposal up to its
// rescaled window, and the reducer that takes all sums of a round at once.  One definition each, so that the pattern, the windows and the
// window-1 update of an L1 run are those of an L2 run bit for bit.
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
    // the L2 norms: (float) sqrt of each sum of squares
    template <class Row>
    __device__ __forceinline__ void norms(int n, float *out, float *__restrict__ global, int64_t B, int64_t b, Row row) {
        sums(n, out, global, B, b, row, [](double r) { return static_cast<float>(sqrt(r)); });
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
struct Tiling {
    int s0, nh, nw, oh, ow;
    int64_t id;
    const float *eta;
    // d of element (c, h, w): +-eta0[r][q], transposed by the tile's coin; 0 outside the tiling
    __device__ __forceinline__ float value(const Philox &ph, int c, int h, int w) const {
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

}  // namespace ee
