// ee_sample.hpp - the "one workgroup of 512 threads per sample" expressions, each written once ("The per-sample
// workgroup kernels").
//
// ee_fab.hip, ee_apgd_l2.hip, ee_apgd_l1.hip, ee_sqatk_l2.hip and ee_sqatk_l1.hip each have a *resident* path (a sample stays in registers across all
// passes, per_sample <= kSampleResident) and a *streaming* path (every pass re-reads its inputs; any size, no scratch tensor), with 16-byte
// or element-wise accesses, and promise the same BITS from all of them.  That holds because every sum over a sample is taken in one order:
//   1. thread t takes the float4 groups t, t + 512, ... in turn (group_element), the four elements of a group in index order; elements at
//      or past D read as 0 and are not written (load4 / store4), so the order depends on D alone, not on the path or the access width;
//   2. a wavefront is reduced by an xor-butterfly (ee_rows.hpp), after which every lane holds the wavefront's result;
//   3. lane 0 of each wavefront stores it to LDS, one barrier, and every thread combines the eight partials in index order.
// Real sums are double (the products, squares and differences of floats they add are exact there), counts are int.  The order above and
// the operand order below are part of the contract, as in ee_rows.hpp.
#pragma once
#include <type_traits>

#include "ee_rows.hpp"

namespace ee {

constexpr int kSampleBlock = 512;                              // 8 wavefronts per sample
constexpr int kSampleWaves = kSampleBlock / kWave;
constexpr int kSampleVecs = 6;                                 // float4 groups per thread the resident path keeps
constexpr int kSampleElems = kSampleVecs * 4;
constexpr int kSampleSlots = kSampleBlock * 4;                 // elements one float4 group per thread covers: 2048
constexpr int kSampleResident = kSampleSlots * kSampleVecs;    // 12288 = 3*64*64

// the element at which this thread's g-th float4 group starts, and the groups per thread that cover D elements (<= kSampleVecs when resident)
__device__ __forceinline__ int64_t group_element(int g) { return (static_cast<int64_t>(g) * kSampleBlock + threadIdx.x) * 4; }
__host__ __device__ __forceinline__ int groups_of(int64_t D) { return static_cast<int>((D + kSampleSlots - 1) / kSampleSlots); }

// four consecutive elements of a row from element e on; elements at or past D read as 0
template <bool VEC>
__device__ __forceinline__ void load4(const float *row, int64_t e, int64_t D, float (&o)[4]) {
    if (VEC && e + 3 < D) {
        const float4 v = *reinterpret_cast<const float4 *>(row + e);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = e + j < D ? row[e + j] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float *row, int64_t e, int64_t D, const float (&v)[4]) {
    if (VEC && e + 3 < D) {
        *reinterpret_cast<float4 *>(row + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < D) row[e + j] = v[j];
    }
}

// ---- the draw of a random start (ee_fab_start_f32 under kStreamFabStart, ee_apgd_start_f32 under kStreamApgdStart) ------------------------
// Four consecutive elements of sample b's draw from element e on.  DRAW: one Philox call per group of four elements under the counter
// (b << 32) | (e >> 2) and the stream id STREAM - a row's draw depends on (seed, b, element) alone - UNIFORM: 2 u01 - 1 on [-1, 1), else
// the standard normals of normal4.  !DRAW: the row of injected noise.  Elements at or past D read as 0 either way, as load4's do.
template <uint32_t STREAM, bool UNIFORM, bool DRAW, bool VEC>
__device__ __forceinline__ void start_draw4(const Philox &ph, const float *noise_row, int b, int64_t e, int64_t D, float (&t)[4]) {
    if (!DRAW) {
        load4<VEC>(noise_row, e, D, t);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = 0.0f;
    if (e >= D) return;  // a group past the row: nothing to draw (e is fixed by the thread and the group, not by data)
    const uint4 r = ph((static_cast<uint64_t>(static_cast<uint32_t>(b)) << 32) | static_cast<uint64_t>(e >> 2), STREAM);
    if (UNIFORM) {
        t[0] = 2.0f * u01(r.x) - 1.0f;  // exact: u01 is a multiple of 2^-24 in [0, 1)
        t[1] = 2.0f * u01(r.y) - 1.0f;
        t[2] = 2.0f * u01(r.z) - 1.0f;
        t[3] = 2.0f * u01(r.w) - 1.0f;
    } else {
        normal4(r, t);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (e + j >= D) t[j] = 0.0f;  // elements at or past D read as 0, as load4's do
}

// the int butterfly (a name of its own: a wave_sum overload declared in a file's own namespace hides ee::wave_sum(double) from it, and
// ee_rows.hpp keeps that name for the double sum alone)
__device__ __forceinline__ int wave_count(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Reductions over the workgroup; every thread gets the result.  Consecutive reductions of a type alternate halves of its buffer, so one
// barrier per reduction is enough: a thread can be at most one reduction ahead of the slowest, and then writes the other half.  The kernel
// declares the arrays; one that sums no ints leaves shi out and pays no LDS for it.
struct SampleReducer {
    double *shd;         // [2][kSampleWaves]
    int *shi = nullptr;  // [2][kSampleWaves]
    int pd = 0, pi = 0;
    template <class T, class C>
    static __device__ __forceinline__ T finish(T v, T *sh, int &phase, C combine) {
        T *buf = sh + phase * kSampleWaves;
        phase ^= 1;
        if ((threadIdx.x & (kWave - 1)) == 0) buf[threadIdx.x >> 6] = v;
        __syncthreads();
        T r = buf[0];
#pragma unroll
        for (int i = 1; i < kSampleWaves; ++i) r = combine(r, buf[i]);
        return r;
    }
    __device__ __forceinline__ double sum(double v) {
        return finish(wave_sum(v), shd, pd, [](double a, double b) { return a + b; });
    }
    __device__ __forceinline__ double max(double v) {
        return finish(wave_max(v), shd, pd, [](double a, double b) { return fmax(a, b); });
    }
    __device__ __forceinline__ int sum(int v) {
        return finish(wave_count(v), shi, pi, [](int a, int b) { return a + b; });
    }
};

// ---- host: (path, per_sample, pointers) -> the <RES, VEC> instantiation ------------------------------------------------------------------
// EE_PATH_* -> *res; a path outside the three: EE_ERR_SHAPE, EE_PATH_RESIDENT past kSampleResident: EE_ERR_UNSUPPORTED
static inline int sample_path(int path, int64_t per_sample, bool *res) {
    if (path < EE_PATH_AUTO || path > EE_PATH_STREAMING) return EE_ERR_SHAPE;
    if (path == EE_PATH_RESIDENT && per_sample > kSampleResident) return EE_ERR_UNSUPPORTED;
    *res = path == EE_PATH_RESIDENT || (path == EE_PATH_AUTO && per_sample <= kSampleResident);
    return EE_OK;
}

// 16-byte accesses: every row of every tensor then starts 16-byte aligned
template <class... P>
static inline bool sample_vec(int64_t per_sample, const P *...tensors) {
    return (per_sample & 3) == 0 && (aligned16(tensors) && ...);
}

// launch(RES, VEC) with the two as constants: in a generic lambda, `kernel<RES, VEC>` names the instantiation
template <class F>
static inline void sample_launch(bool res, bool vec, F launch) {
    if (res && vec)
        launch(std::true_type{}, std::true_type{});
    else if (res)
        launch(std::true_type{}, std::false_type{});
    else if (vec)
        launch(std::false_type{}, std::true_type{});
    else
        launch(std::false_type{}, std::false_type{});
}

}  // namespace ee
