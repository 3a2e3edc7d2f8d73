// ee_cascade.hip - device-resident sample pools of the survivor-only attack cascade (gfx950).
//
// A pool is a row store of fixed capacity: x [cap, D] f32, label [cap] i64, sample id [cap] i64, class order [cap, K] i64 and one
// count (i32) on the device.  Three operations, all of them pure memory traffic:
//   append   rows b of a batch with keep[b] != 0 go behind the count rows already there, in source order        (copy, then count)
//   pop      the first B rows go to the batch buffers, the rest (fewer than B) moves to the front                (copy, move, then count)
//   resolve  what a stage broke is written to robust_out / stage_out / adv_out by sample id; keep <- survived    (one launch)
// The count is read by the copying launches and advanced by a tiny launch of its own after them: no workgroup reads a scalar that
// another workgroup of the same launch writes.  A kept row's rank among the kept rows is counted inside its own workgroups from
// keep[0 .. b).  Every loop's trip count follows from the launch shape, b and D, never from the data.
//
// Rows are copied as bits (uint32 / uint4: NaNs keep their payloads).  One grid row of workgroups per batch row, the row's D words
// split over gridDim.x workgroups: 16-byte accesses where BOTH row starts are 16-byte aligned (decided per row: with D % 4 != 0 every
// other pool row is not), word by word otherwise.
#include "ee_common.hpp"

namespace {

using namespace ee;

constexpr int kMaxChunks = 32;  // workgroups per row at most; a longer row is covered by the grid-stride loop

__device__ __forceinline__ bool aligned16_dev(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the part of row src -> dst [D words] of workgroup blockIdx.x (of gridDim.x)
__device__ __forceinline__ void copy_row(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int64_t D) {
    const int64_t t0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    if (aligned16_dev(src) && aligned16_dev(dst)) {  // uniform over the workgroup
        const int64_t D4 = D / 4;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int64_t i = t0; i < D4; i += stride) d4[i] = s4[i];
        for (int64_t i = 4 * D4 + t0; i < D; i += stride) dst[i] = src[i];  // the D % 4 words of the tail
    } else {
        for (int64_t i = t0; i < D; i += stride) dst[i] = src[i];
    }
}

// label, id and class order of one row: workgroup blockIdx.x == 0 of the row
__device__ __forceinline__ void copy_fields(const int64_t *y, const int64_t *id, const int64_t *order, int64_t s, int64_t *y_out, int64_t *id_out,
                                            int64_t *order_out, int64_t d, int K) {
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) y_out[d] = y[s], id_out[d] = id[s];
    for (int k = threadIdx.x; k < K; k += blockDim.x) order_out[d * K + k] = order[s * K + k];
}

__device__ __forceinline__ int64_t clamp_count(const int32_t *count, int64_t cap) {
    const int64_t c = *count;
    return c < 0 ? 0 : (c > cap ? cap : c);
}

// workgroups (., b): batch row b, if kept, -> pool row count + #{i < b : keep[i]}
__global__ __launch_bounds__(kBlock) void pool_append_kernel(const uint32_t *__restrict__ x, const int64_t *__restrict__ y,
                                                             const int64_t *__restrict__ id, const int64_t *__restrict__ order,
                                                             const uint8_t *__restrict__ keep, int64_t D, int K, uint32_t *__restrict__ pool_x,
                                                             int64_t *__restrict__ pool_y, int64_t *__restrict__ pool_id,
                                                             int64_t *__restrict__ pool_order, const int32_t *__restrict__ count, int64_t cap) {
    const int b = blockIdx.y;
    if (keep[b] == 0) return;
    int rank = 0;
    for (int i0 = 0; i0 < b; i0 += kBlock) {  // ceil(b / kBlock) trips, the same for every thread of the workgroup
        const int i = i0 + static_cast<int>(threadIdx.x);
        rank += __syncthreads_count(i < b && keep[i] != 0);
    }
    const int64_t d = clamp_count(count, cap) + rank;
    if (d >= cap) return;  // the host keeps this from happening; never written out of bounds
    copy_row(x + b * D, pool_x + d * D, D);
    copy_fields(y, id, order, b, pool_y, pool_id, pool_order, d, K);
}

// one workgroup: count <- min(count + #{i < B : keep[i]}, cap) (keep given), or count <- min(max(count - B, 0), B) (keep == nullptr)
__global__ __launch_bounds__(kBlock) void pool_count_kernel(const uint8_t *__restrict__ keep, int B, int32_t *__restrict__ count, int64_t cap) {
    int kept = 0;
    if (keep != nullptr) {
        for (int i0 = 0; i0 < B; i0 += kBlock) {
            const int i = i0 + static_cast<int>(threadIdx.x);
            kept += __syncthreads_count(i < B && keep[i] != 0);
        }
    }
    if (threadIdx.x == 0) {
        const int64_t c = clamp_count(count, cap);
        int64_t n = keep != nullptr ? c + kept : c - B;
        if (keep == nullptr && n > B) n = B;  // only B rows were moved to the front
        *count = static_cast<int32_t>(n < 0 ? 0 : (n > cap ? cap : n));
    }
}

// workgroups (., r): pool row (r < count ? r : 0) -> batch row r; a pool with fewer than B rows pads the batch with its row 0
__global__ __launch_bounds__(kBlock) void pool_pop_kernel(const uint32_t *__restrict__ pool_x, const int64_t *__restrict__ pool_y,
                                                          const int64_t *__restrict__ pool_id, const int64_t *__restrict__ pool_order,
                                                          const int32_t *__restrict__ count, int64_t cap, int64_t D, int K,
                                                          uint32_t *__restrict__ x, int64_t *__restrict__ y, int64_t *__restrict__ id,
                                                          int64_t *__restrict__ order) {
    const int64_t r = blockIdx.y;
    const int64_t s = r < clamp_count(count, cap) ? r : 0;
    copy_row(pool_x + s * D, x + r * D, D);
    copy_fields(pool_y, pool_id, pool_order, s, y, id, order, r, K);
}

// workgroups (., r): pool row B + r -> pool row r where B + r < count.  Reads rows [B, 2B), writes rows [0, B): disjoint.
__global__ __launch_bounds__(kBlock) void pool_front_kernel(uint32_t *pool_x, int64_t *pool_y, int64_t *pool_id, int64_t *pool_order,
                                                            const int32_t *__restrict__ count, int64_t cap, int64_t D, int K, int B) {
    const int64_t r = blockIdx.y;
    const int64_t s = B + r;
    if (s >= clamp_count(count, cap)) return;
    copy_row(pool_x + s * D, pool_x + r * D, D);
    copy_fields(pool_y, pool_id, pool_order, s, pool_y, pool_id, pool_order, r, K);
}

// workgroups (., b): row b < n_valid with an id in [0, N) is a sample of the stage: keep[b] <- robust[b]; a broken one is recorded
__global__ __launch_bounds__(kBlock) void cascade_resolve_kernel(const uint8_t *__restrict__ robust, const int64_t *__restrict__ id,
                                                                 const uint32_t *__restrict__ x_adv, int n_valid, int64_t D, int stage,
                                                                 int64_t N, uint8_t *__restrict__ robust_out, int32_t *__restrict__ stage_out,
                                                                 uint32_t *__restrict__ adv_out, uint8_t *__restrict__ keep) {
    const int b = blockIdx.y;
    const int64_t n = id[b];
    const bool valid = b < n_valid && n >= 0 && n < N;
    const bool survived = robust[b] != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        keep[b] = valid && survived ? 1 : 0;
        if (valid && !survived) robust_out[n] = 0, stage_out[n] = stage;
    }
    if (valid && !survived && adv_out != nullptr) copy_row(x_adv + b * D, adv_out + n * D, D);
}

dim3 row_grid(int rows, int64_t D) {
    int64_t chunks = (D / 4 + kBlock - 1) / kBlock;  // sized for the 16-byte path
    chunks = chunks < 1 ? 1 : (chunks > kMaxChunks ? kMaxChunks : chunks);
    return dim3(static_cast<unsigned>(chunks), static_cast<unsigned>(rows));
}

bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

int check_shape(int B, long long D, int K, long long cap) {
    if (B < 1 || D < 1 || K < 1 || cap < 1) return EE_ERR_SHAPE;
    if (B > 4096 || cap > 0x7fffffffLL || K > 4096) return EE_ERR_UNSUPPORTED;
    return EE_OK;
}

}  // namespace

EE_API int ee_pool_append_f32(const float *x, const int64_t *y, const int64_t *id, const int64_t *order, const uint8_t *keep, int B, long long D,
                              int K, float *pool_x, int64_t *pool_y, int64_t *pool_id, int64_t *pool_order, int32_t *count, long long cap,
                              void *stream) {
    if (const int rc = check_shape(B, D, K, cap)) return rc;
    if (!x || !y || !id || !order || !keep || !pool_x || !pool_y || !pool_id || !pool_order || !count) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(pool_x) || !aligned4(count) || !aligned8(y) || !aligned8(id) || !aligned8(order) || !aligned8(pool_y) ||
        !aligned8(pool_id) || !aligned8(pool_order))
        return EE_ERR_ALIGN;
    EE_LAUNCH(pool_append_kernel, row_grid(B, D), dim3(kBlock), 0, as_stream(stream), reinterpret_cast<const uint32_t *>(x), y, id, order, keep,
              static_cast<int64_t>(D), K, reinterpret_cast<uint32_t *>(pool_x), pool_y, pool_id, pool_order, count, static_cast<int64_t>(cap));
    if (const int rc = launch_status()) return rc;
    EE_LAUNCH(pool_count_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), keep, B, count, static_cast<int64_t>(cap));
    return launch_status();
}

EE_API int ee_pool_pop_f32(float *pool_x, int64_t *pool_y, int64_t *pool_id, int64_t *pool_order, int32_t *count, long long cap, int B,
                           long long D, int K, float *x, int64_t *y, int64_t *id, int64_t *order, void *stream) {
    if (const int rc = check_shape(B, D, K, cap)) return rc;
    if (cap < 2LL * B) return EE_ERR_SHAPE;
    if (!x || !y || !id || !order || !pool_x || !pool_y || !pool_id || !pool_order || !count) return EE_ERR_NULL;
    if (!aligned4(x) || !aligned4(pool_x) || !aligned4(count) || !aligned8(y) || !aligned8(id) || !aligned8(order) || !aligned8(pool_y) ||
        !aligned8(pool_id) || !aligned8(pool_order))
        return EE_ERR_ALIGN;
    const dim3 grid = row_grid(B, D);
    EE_LAUNCH(pool_pop_kernel, grid, dim3(kBlock), 0, as_stream(stream), reinterpret_cast<const uint32_t *>(pool_x), pool_y, pool_id, pool_order,
              count, static_cast<int64_t>(cap), static_cast<int64_t>(D), K, reinterpret_cast<uint32_t *>(x), y, id, order);
    if (const int rc = launch_status()) return rc;
    EE_LAUNCH(pool_front_kernel, grid, dim3(kBlock), 0, as_stream(stream), reinterpret_cast<uint32_t *>(pool_x), pool_y, pool_id, pool_order, count,
              static_cast<int64_t>(cap), static_cast<int64_t>(D), K, B);
    if (const int rc = launch_status()) return rc;
    EE_LAUNCH(pool_count_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), static_cast<const uint8_t *>(nullptr), B, count,
              static_cast<int64_t>(cap));
    return launch_status();
}

EE_API int ee_cascade_resolve_f32(const uint8_t *robust, const int64_t *id, const float *x_adv, int B, int n_valid, long long D, int stage,
                                  long long N, uint8_t *robust_out, int32_t *stage_out, float *adv_out, uint8_t *keep, void *stream) {
    if (B < 1 || D < 1 || N < 1 || n_valid < 0 || n_valid > B) return EE_ERR_SHAPE;
    if (B > 4096) return EE_ERR_UNSUPPORTED;
    if (!robust || !id || !robust_out || !stage_out || !keep || (adv_out && !x_adv)) return EE_ERR_NULL;
    if (!aligned8(id) || !aligned4(stage_out) || !aligned4(x_adv) || !aligned4(adv_out)) return EE_ERR_ALIGN;
    const dim3 grid = adv_out ? row_grid(B, D) : dim3(1, static_cast<unsigned>(B));
    EE_LAUNCH(cascade_resolve_kernel, grid, dim3(kBlock), 0, as_stream(stream), robust, id, reinterpret_cast<const uint32_t *>(x_adv), n_valid,
              static_cast<int64_t>(D), stage, static_cast<int64_t>(N), robust_out, stage_out, reinterpret_cast<uint32_t *>(adv_out), keep);
    return launch_status();
}
