// ee_fd.hip - the dot-product non-local ("feature denoising") product of the resnet*_fd models (ImageNet/models_imagenet/resnet_fd.py:126-148,
// always built with embed=False, softmax=False): per sample, with X the C x P matrix of the map (P = H * W, rows contiguous),
//   forward    F  = scale * X X^T X
//   backward   dX = scale * [ (M + M^T) X + G D ],  G = X X^T, M = D X^T     channel form, C <= P  (d = C)
//              dX = scale * [ D A + X (B + B^T) ],  A = X^T X, B = D^T X     spatial form, C >  P  (d = P)
// Both forms are the same polynomial; the reference picks the association by n_in > H * W, and so does this file (C > P -> spatial).
//
// Each direction is a Gram-type product contracted over the LONG dimension (d x d result, d = min(C, P) <= 256), then an apply whose
// contraction is the short one.  Three launches each way, all of ONE tile kernel (fd_tile_kernel):
//   1. the Gram-type product, its contraction split over `S` workgroups per (sample, 64 x 64 result tile) - 32 samples alone do not fill
//      256 CUs - each split writing its partial tile to scratch (no atomics);
//   2. fd_reduce_kernel adds the S partials in split order (the backward also forms M + M^T here, so the sum is symmetric to the bit);
//      with S == 1 the forward's Gram kernel writes gram directly and this launch is skipped;
//   3. the apply: a 64 x 64 tile of the C x P result per workgroup, the d-long contraction walked in rounds of 32 through LDS (a 256 x 256
//      operand is 256 KB and never sits in LDS whole); the backward runs its two products into the same accumulators.
// A workgroup is four wavefronts, each owning a 32 x 32 quadrant as 2 x 2 mfma_f32_16x16x4f32 tiles (fragment layout as in ee_dense.hip:
// operand lane = (row | column) l15, k = lane >> 4; result row = 4 (lane >> 4) + register, column = l15).  Both operand tiles sit in LDS as
// [row][k] with stride 36: the 64 lanes of an operand read fall on 64 distinct banks.
// Every element is loaded on its own with a bounds check and zero fill, so ragged edges (P = 35, 49, 196, 1), splits that do not divide the
// contraction and base pointers off 16 bytes all take the same code and give the same bits.  The order of every sum is fixed by the shape
// alone: results are bit-identical run to run.  `scale` multiplies the finished sum once.
//
// CNN-body glue, not a row of SURVEY.md section 8.
#include "ee_common.hpp"

namespace {

using namespace ee;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FD_NT = 256;         // four wavefronts
constexpr int FD_T = 64;           // result tile: 64 x 64
constexpr int FD_KU = 32;          // contraction indices per round
constexpr int FD_SK = FD_KU + 4;   // LDS row stride: bank = (36 row + k) % 64, distinct over the 16 rows x 4 k of an operand read
constexpr int FD_MAX_D = 256, FD_MAX_C = 2048, FD_MAX_P = 4096;
constexpr int FD_TARGET_WG = 512;  // workgroups the split Gram product aims at (two per CU)

// element (row, k) of an operand sits at p + batch * n + row * rs + k * ks
struct FdOperand {
    const float *p;
    int64_t batch;
    int rs, ks;
};

struct FdTile {
    FdOperand a1, b1, a2, b2;  // result = scale * (A1 B1^T [+ A2 B2^T]) with both operands as [row][k]; a2.p == nullptr: one product
    float *out;                // result (m, n) at out + out_batch * sample + out_split * split + m * out_rs + n
    int64_t out_batch, out_split;
    int out_rs;
    int M, N, K;               // result rows / columns, contraction length
    int kchunk;                // contraction indices per split (a multiple of FD_KU); gridDim.y splits
    float scale;
};

// one operand tile of a round into LDS: tile[row][k] = src(row0 + row, k0 + k), zero outside [0, R) x [k0, kend)
// KC: k is the contiguous index in memory (ks == 1): 32 consecutive floats per row; else the row index is (rs == 1): 64 consecutive floats per k
template <bool KC>
__device__ __forceinline__ void fd_fetch(float (&v)[8], const float *src, int row0, int R, int rs, int k0, int kend, int ks) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = row0 + (KC ? (tid >> 5) + 8 * j : (tid & 63));
        const int k = k0 + (KC ? (tid & 31) : (tid >> 6) + 4 * j);
        v[j] = (row < R && k < kend) ? src[static_cast<size_t>(row) * rs + static_cast<size_t>(k) * ks] : 0.0f;
    }
}
template <bool KC>
__device__ __forceinline__ void fd_store(float *tile, const float (&v)[8]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = KC ? (tid >> 5) + 8 * j : (tid & 63);
        const int k = KC ? (tid & 31) : (tid >> 6) + 4 * j;
        tile[row * FD_SK + k] = v[j];
    }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(FD_NT) void fd_tile_kernel(FdTile t) {
    __shared__ float as[FD_T * FD_SK], bs[FD_T * FD_SK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, lq = lane >> 4;
    const int ntiles = (t.N + FD_T - 1) / FD_T;
    const int mt = blockIdx.x / ntiles, nt = blockIdx.x - mt * ntiles;
    const int m0 = mt * FD_T, n0 = nt * FD_T;
    const int split = blockIdx.y, sample = blockIdx.z;
    const int kbeg = split * t.kchunk;
    const int kend = kbeg + t.kchunk < t.K ? kbeg + t.kchunk : t.K;
    const int wm = 32 * (wave >> 1), wn = 32 * (wave & 1);

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int products = t.a2.p ? 2 : 1;
    for (int pr = 0; pr < products; ++pr) {
        const FdOperand &oa = pr ? t.a2 : t.a1, &ob = pr ? t.b2 : t.b1;
        const float *ap = oa.p + oa.batch * sample, *bp = ob.p + ob.batch * sample;
        float va[8], vb[8];
        fd_fetch<A_KC>(va, ap, m0, t.M, oa.rs, kbeg, kend, oa.ks);
        fd_fetch<B_KC>(vb, bp, n0, t.N, ob.rs, kbeg, kend, ob.ks);
        for (int k0 = kbeg; k0 < kend; k0 += FD_KU) {
            __syncthreads();  // the previous round's operand reads are done
            fd_store<A_KC>(as, va);
            fd_store<B_KC>(bs, vb);
            __syncthreads();
            if (k0 + FD_KU < kend) {  // the next round travels while this one is multiplied
                fd_fetch<A_KC>(va, ap, m0, t.M, oa.rs, k0 + FD_KU, kend, oa.ks);
                fd_fetch<B_KC>(vb, bp, n0, t.N, ob.rs, k0 + FD_KU, kend, ob.ks);
            }
            const float *ar = as + (wm + l15) * FD_SK + lq, *br = bs + (wn + l15) * FD_SK + lq;
#pragma unroll
            for (int s = 0; s < FD_KU / 4; ++s) {
                const float a0 = ar[4 * s], a1 = ar[16 * FD_SK + 4 * s];
                const float b0 = br[4 * s], b1 = br[16 * FD_SK + 4 * s];
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    float *op = t.out + t.out_batch * sample + t.out_split * split;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * lq + r, n = n0 + wn + 16 * j + l15;
                if (m < t.M && n < t.N) op[static_cast<size_t>(m) * t.out_rs + n] = acc[i][j][r] * t.scale;
            }
}

// out[n][i][j] = sum_s part[n][s][i][j] (+ sum_s part[n][s][j][i] with SYM), the splits added in order
template <bool SYM>
__global__ __launch_bounds__(kBlock) void fd_reduce_kernel(const float *__restrict__ part, float *__restrict__ out, int64_t total, int d, int S) {
    const int64_t dd = static_cast<int64_t>(d) * d;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlock) {
        const int64_t n = e / dd, r = e - n * dd;
        const float *p = part + n * S * dd;
        float s = p[r];
        for (int k = 1; k < S; ++k) s += p[k * dd + r];
        if constexpr (SYM) {
            const int i = static_cast<int>(r / d), j = static_cast<int>(r - static_cast<int64_t>(i) * d);
            const int64_t rt = static_cast<int64_t>(j) * d + i;
            float u = p[rt];
            for (int k = 1; k < S; ++k) u += p[k * dd + rt];
            s += u;  // (i, j) and (j, i) add the same two sums: symmetric to the bit
        }
        out[e] = s;
    }
}

bool fd_class(int C, int P) {
    return C >= 64 && C % 64 == 0 && C <= FD_MAX_C && P >= 1 && P <= FD_MAX_P && (C < P ? C : P) <= FD_MAX_D;
}

struct FdPlan {
    bool spatial;
    int d, L, S, kchunk;
};

// the split of the long contraction: a function of the shape alone, so the summation order is too
FdPlan fd_plan(int N, int C, int P) {
    FdPlan p;
    p.spatial = C > P;
    p.d = p.spatial ? P : C;
    p.L = p.spatial ? C : P;
    const int tiles = ((p.d + FD_T - 1) / FD_T) * ((p.d + FD_T - 1) / FD_T);
    const int64_t base = static_cast<int64_t>(N < 1 ? 1 : N) * tiles;
    int64_t want = (FD_TARGET_WG + base - 1) / base;
    const int maxs = (p.L + 2 * FD_KU - 1) / (2 * FD_KU);  // at least two rounds per split
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    const int per = (p.L + static_cast<int>(want) - 1) / static_cast<int>(want);
    p.kchunk = (per + FD_KU - 1) / FD_KU * FD_KU;
    p.S = (p.L + p.kchunk - 1) / p.kchunk;
    return p;
}

int fd_check(const void *const *ptrs, int nptr, int N, int C, int P, float scale) {
    if (N < 0 || C < 1 || P < 1 || !(scale == scale)) return EE_ERR_SHAPE;
    if (!fd_class(C, P)) return EE_ERR_UNSUPPORTED;
    if (N > 65535 || static_cast<int64_t>(N) * C * P > 0x7fffffffLL) return EE_ERR_SHAPE;
    if (N == 0) return EE_OK;
    for (int i = 0; i < nptr; ++i) {
        if (!ptrs[i]) return EE_ERR_NULL;
        if (!aligned4(ptrs[i])) return EE_ERR_ALIGN;
    }
    return EE_OK;
}

template <bool A_KC, bool B_KC>
int fd_launch(const FdTile &t, int N, int splits, hipStream_t st) {
    const unsigned tiles = static_cast<unsigned>((t.M + FD_T - 1) / FD_T) * static_cast<unsigned>((t.N + FD_T - 1) / FD_T);
    EE_LAUNCH((fd_tile_kernel<A_KC, B_KC>), dim3(tiles, static_cast<unsigned>(splits), static_cast<unsigned>(N)), dim3(FD_NT), 0, st, t);
    return launch_status();
}

// the Gram-type product U V^T (channel form) or U^T V (spatial form) of two C x P maps, split over the long dimension
int fd_gram(const float *u, const float *v, float *out, bool to_scratch, const FdPlan &pl, int N, int C, int P, hipStream_t st) {
    const int64_t cp = static_cast<int64_t>(C) * P, dd = static_cast<int64_t>(pl.d) * pl.d;
    FdTile t{};
    t.out = out;
    t.out_batch = to_scratch ? pl.S * dd : dd, t.out_split = to_scratch ? dd : 0, t.out_rs = pl.d;
    t.M = t.N = pl.d, t.K = pl.L, t.kchunk = pl.kchunk, t.scale = 1.0f;
    if (!pl.spatial) {  // rows are channels, k runs along the contiguous pixels
        t.a1 = FdOperand{u, cp, P, 1}, t.b1 = FdOperand{v, cp, P, 1};
        return fd_launch<true, true>(t, N, pl.S, st);
    }
    t.a1 = FdOperand{u, cp, 1, P}, t.b1 = FdOperand{v, cp, 1, P};  // rows are pixels, k runs down the channels
    return fd_launch<false, false>(t, N, pl.S, st);
}

template <bool SYM>
int fd_reduce(const float *part, float *out, const FdPlan &pl, int N, hipStream_t st) {
    const int64_t total = static_cast<int64_t>(N) * pl.d * pl.d;
    EE_LAUNCH((fd_reduce_kernel<SYM>), dim3(grid_for(total)), dim3(kBlock), 0, st, part, out, total, pl.d, pl.S);
    return launch_status();
}

// out [C x P] = scale * (small . big [+ small2 . big2]) (channel form) or scale * (big . small [+ big2 . small2]) (spatial form);
// small operands are d x d, symmetric or not: element (row, k) is read as written
int fd_apply(const float *small1, const float *big1, const float *small2, const float *big2, float *out, float scale, const FdPlan &pl, int N, int C, int P,
             hipStream_t st) {
    const int64_t cp = static_cast<int64_t>(C) * P, dd = static_cast<int64_t>(pl.d) * pl.d;
    FdTile t{};
    t.out = out, t.out_batch = cp, t.out_split = 0, t.out_rs = P;
    t.M = C, t.N = P, t.K = pl.d, t.kchunk = (pl.d + FD_KU - 1) / FD_KU * FD_KU, t.scale = scale;
    if (!pl.spatial) {  // out[i][p] = sum_j small[i][j] big[j][p]: A = small (k contiguous), B rows are pixels (row index contiguous)
        t.a1 = FdOperand{small1, dd, pl.d, 1}, t.b1 = FdOperand{big1, cp, 1, P};
        if (small2) t.a2 = FdOperand{small2, dd, pl.d, 1}, t.b2 = FdOperand{big2, cp, 1, P};
    } else {            // out[c][p] = sum_q big[c][q] small[q][p]
        t.a1 = FdOperand{big1, cp, P, 1}, t.b1 = FdOperand{small1, dd, 1, pl.d};
        if (small2) t.a2 = FdOperand{big2, cp, P, 1}, t.b2 = FdOperand{small2, dd, 1, pl.d};
    }
    return fd_launch<true, false>(t, N, 1, st);
}

}  // namespace

EE_API int ee_fd_supported(int C, int P) { return fd_class(C, P) ? 1 : 0; }

// floats of scratch for either direction: S partial d x d tiles per sample, and the backward's symmetrised sum
EE_API int64_t ee_fd_scratch_floats(int N, int C, int P) {
    if (N < 1 || !fd_class(C, P)) return 0;
    const FdPlan pl = fd_plan(N, C, P);
    return static_cast<int64_t>(N) * pl.d * pl.d * (pl.S + 1);
}

EE_API int ee_fd_fwd_f32(const float *x, float *f, float *gram, float *scratch, int N, int C, int P, float scale, void *stream) {
    const void *ptrs[] = {x, f, gram, scratch};
    const int rc = fd_check(ptrs, 4, N, C, P, scale);
    if (rc != EE_OK || N == 0) return rc;
    if (f == x) return EE_ERR_SHAPE;
    const FdPlan pl = fd_plan(N, C, P);
    hipStream_t st = as_stream(stream);
    int e = fd_gram(x, x, pl.S > 1 ? scratch : gram, pl.S > 1, pl, N, C, P, st);
    if (e != EE_OK) return e;
    if (pl.S > 1 && (e = fd_reduce<false>(scratch, gram, pl, N, st)) != EE_OK) return e;
    return fd_apply(gram, x, nullptr, nullptr, f, scale, pl, N, C, P, st);
}

EE_API int ee_fd_bwd_f32(const float *x, const float *df, const float *gram, float *dx, float *scratch, int N, int C, int P, float scale, void *stream) {
    const void *ptrs[] = {x, df, gram, dx, scratch};
    const int rc = fd_check(ptrs, 5, N, C, P, scale);
    if (rc != EE_OK || N == 0) return rc;
    if (dx == x || dx == df) return EE_ERR_SHAPE;
    const FdPlan pl = fd_plan(N, C, P);
    hipStream_t st = as_stream(stream);
    float *sym = scratch + static_cast<int64_t>(N) * pl.d * pl.d * pl.S;
    int e = fd_gram(df, x, scratch, true, pl, N, C, P, st);  // M = D X^T, or B = D^T X
    if (e != EE_OK) return e;
    if ((e = fd_reduce<true>(scratch, sym, pl, N, st)) != EE_OK) return e;
    // channel: (M + M^T) X + G D; spatial: D A + X (B + B^T)
    if (!pl.spatial) return fd_apply(sym, x, gram, df, dx, scale, pl, N, C, P, st);
    return fd_apply(gram, df, sym, x, dx, scale, pl, N, C, P, st);
}
