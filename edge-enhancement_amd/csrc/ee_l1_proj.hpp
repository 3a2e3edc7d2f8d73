// ee_l1_proj.hpp - the exact Euclidean projection onto {z : ||z - x0||_1 <= eps} n [0,1]^D of one sample, written once (DESIGN.md
// sections 19 and 21): the coordinate, the search for the multiplier with its segment solve, and the pass that writes the point.
// ee_apgd_l1.hip (ee_l1_proj_f32, ee_apgd_step_l1_f32) and ee_sqatk_l1.hip (the Square-L1 start and step) run it inside their own
// launches, each over its own way of visiting a sample's coordinates:
//     each(body)  calls  body(e, w[4], lo[4], x0[4])  for every float4 group of the thread, in the order of ee_sample.hpp, zeros past D
// - from registers on a resident path (l1_each_resident), recomputed from the launch's inputs on a streaming one.  The sums are double
// in that one order and the reductions are SampleReducer's, so what a launch returns depends on (w, lo, x0, eps) alone.
#pragma once
#include <math.h>

#include "ee_sample.hpp"

namespace ee {

__device__ __forceinline__ uint32_t abs_bits(float g) { return __float_as_uint(g) & 0x7FFFFFFFu; }

// one coordinate of the projection problem: a = |u - x0|, lo = how far u lies outside the box (never above a), w keeps the sign
struct L1Coord {
    float w, a, lo;
    __device__ __forceinline__ L1Coord(float w_, float lo_) : w(w_), a(fabsf(w_)), lo(lo_) {}
    static __device__ __forceinline__ L1Coord of(float u, float x0) {
        const float w = u - x0;
        return L1Coord(w, fminf(fmaxf(0.0f, -fminf(1.0f - u, u)), fabsf(w)));
    }
    __device__ __forceinline__ float cut(float lam) const { return fminf(fmaxf(lam, lo), a); }  // min(max(lambda, lo), a)
    __device__ __forceinline__ float point(float x0, float lam) const { return tclamp(x0 + sgn(w) * (a - cut(lam)), 0.0f, 1.0f); }
};

// the resident visit: the groups live in rw / rl / rc
template <class F>
__device__ __forceinline__ void l1_each_resident(const float (&rw)[kSampleElems], const float (&rl)[kSampleElems],
                                                 const float (&rc)[kSampleElems], F body) {
#pragma unroll
    for (int g = 0; g < kSampleVecs; ++g) {
        float wv[4] = {rw[g * 4], rw[g * 4 + 1], rw[g * 4 + 2], rw[g * 4 + 3]};
        float lv[4] = {rl[g * 4], rl[g * 4 + 1], rl[g * 4 + 2], rl[g * 4 + 3]};
        const float cv[4] = {rc[g * 4], rc[g * 4 + 1], rc[g * 4 + 2], rc[g * 4 + 3]};
        // the values are handed over opaquely: what a pass derives from them (their doubles above all) is then formed inside the pass
        // and not kept in registers across the 31 passes of a search, which would not fit
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(wv[j]), "+v"(lv[j]));
        body(group_element(g), wv, lv, cv);
    }
}

// what the search leaves: rest (u - x0 is not finite somewhere: the sample is written as x0), h(0), lambda, |A|
struct L1Root {
    bool rest;
    double h0;
    float lam;
    int active;
};

// lambda = 0 when h(0) <= eps, else the root of h(lambda) = sum_i (a_i - min(max(lambda, lo_i), a_i)) = eps: T, the largest float with
// h(T) > eps, by 31 steps over the bit pattern of non-negative floats (one workgroup-wide sum each), then the segment (T, T+] in closed form
template <class Each>
__device__ __forceinline__ L1Root l1_root(SampleReducer &red, float eps, Each each) {
    // h(0) and whether u - x0 is finite everywhere
    double acc = 0.0;
    int bad = 0;
    each([&](int64_t, const float(&wv)[4], const float(&lv)[4], const float(&)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const L1Coord c(wv[j], lv[j]);
            bad += abs_bits(c.w) >= 0x7F800000u ? 1 : 0;
            acc += static_cast<double>(c.a) - static_cast<double>(c.lo);
        }
    });
    const bool rest = red.sum(bad) != 0;  // a non-finite u: the sample is written as x0
    const double h0 = red.sum(acc), epsd = static_cast<double>(eps);
    float lam = 0.0f;
    int active = 0;
    if (!rest && h0 > epsd) {
        // T: the largest non-negative float with h(T) > eps.  h(0) > eps holds and h(+inf) = 0 does not, so T stays finite.
        uint32_t T = 0u;
#pragma unroll 1
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            const float tf = __uint_as_float(cand);
            double part = 0.0;
            each([&](int64_t, const float(&wv)[4], const float(&lv)[4], const float(&)[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const L1Coord c(wv[j], lv[j]);
                    part += static_cast<double>(c.a) - static_cast<double>(c.cut(tf));
                }
            });
            if (red.sum(part) > epsd) T = cand;
        }
        // the segment (T, T+]: h(lambda) = num - |A| lambda there
        const float tl = __uint_as_float(T), tn = __uint_as_float(T + 1u);
        double num = 0.0;
        int cnt = 0;
        each([&](int64_t, const float(&wv)[4], const float(&lv)[4], const float(&)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const L1Coord c(wv[j], lv[j]);
                if (c.a > tl) {
                    if (c.lo > tl) {
                        num += static_cast<double>(c.a) - static_cast<double>(c.lo);
                    } else {
                        num += static_cast<double>(c.a);
                        ++cnt;
                    }
                }
            }
        });
        num = red.sum(num);
        active = red.sum(cnt);
        lam = active > 0 ? fminf(fmaxf(static_cast<float>((num - epsd) / static_cast<double>(active)), tl), tn) : tn;
    }
    return L1Root{rest, h0, lam, active};
}

// the final pass: store(e, r[4]) takes every group's point, each element from the thread that read it; returns ||z - x0||_1
template <class Each, class Store>
__device__ __forceinline__ double l1_write(SampleReducer &red, const L1Root &root, Each each, Store store) {
    double dist = 0.0;
    each([&](int64_t e, const float(&wv)[4], const float(&lv)[4], const float(&cv)[4]) {
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = root.rest ? cv[j] : L1Coord(wv[j], lv[j]).point(cv[j], root.lam);
            dist += fabs(static_cast<double>(r[j]) - static_cast<double>(cv[j]));
        }
        store(e, r);
    });
    return red.sum(dist);
}

// rows EE_L1_S_LAMBDA .. _DIST of scal [>= 4, B] for sample b (one thread calls it)
__device__ __forceinline__ void l1_scal(float *scal, int64_t B, int64_t b, const L1Root &root, double dist) {
    scal[b] = root.lam;
    scal[B + b] = root.rest ? INFINITY : static_cast<float>(root.h0);
    scal[2 * B + b] = static_cast<float>(root.active);
    scal[3 * B + b] = static_cast<float>(dist);
}

}  // namespace ee
