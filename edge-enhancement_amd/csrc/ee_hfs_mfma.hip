// ee_hfs_mfma.hip - HighFreqSuppress (utils/core.py:15-55) for planes past ee_hfs.hip's 64 x 64 on the f32 matrix cores: one
// workgroup per plane, the plane cut into 16-row bands, BPW consecutive bands per wavefront.  One kernel serves two plane classes:
//     narrow  ee_hfs_mfma_f32  up to 256 x 256 (ImageNet: 224 x 224, r = 16): BPW = 1, [P | Q] 32 columns (NT = 2), MT2 = 2 or 4
//     wide    ee_hfs_wide_f32  up to 320 x 320 (ImageNet/fgsm_imagenet phase 3: 288 x 288, r = 18): BPW = 2 (288 rows are 18 bands
//                              and a workgroup has at most 16 wavefronts), [P | Q] 32 or 64 columns (NT = 2 or 4), MT2 = 2, 4 or 6
//
// ee_hfs.hip keeps a whole plane in LDS and is limited to 64 x 64; beyond that the host layer used three rocBLAS launches and a
// [B,C,H,2W] intermediate in HBM.  The operator is still the rank-(NU x 2NV) one (eeadv/hfs.py), so here it is the same four
// skinny products as in ee_chain.hip, chained through the v_mfma_f32_16x16x4_f32 accumulators, but split over the bands:
//     S1  [P | Q]   = X_band  T1                 per band: 16 x W times W x 16 NT   (X staged through a wave-private LDS strip)
//     S2  R_band    = CS_band^T [P | Q]          per band: 2NU x 16 times 16 x 16 NT -> a wavefront's bands accumulate into the
//                                                same MT2 x NT tiles; summed over the wavefronts through LDS
//     EF            = (a - d | c + b ; b + c | d - a)                                   (tile-wise register arithmetic)
//     S3  [U | V]^T = EF^T CS_band^T / H         per band
//     S4  y_band    = [U | V] T4                 per band: 16 x 16 NT times 16 NT x W
// scripts/chain_emulate.py (wide_tables / wide_apply, with the narrow class as its NT = 2, BPW = 1 case) is the specification of
// the fragment-ordered tables and checks the index algebra against the dense operator in float64.  HBM traffic = the algorithmic
// minimum, read x + write y (8 B per element; 12 with sq_mode 2).  The reduction over the wavefronts goes through the strips four
// tiles at a time and adds each element in wavefront order = band order: results are bit-reproducible run to run.
//
// sq_mode as in ee_hfs_f32: 1 applies Add_Square (core.py:636-655) while a strip is staged, 2 multiplies the result by
// d add_square / dx evaluated at sq_x.  Parity: UNPINNED like ee_hfs.hip (torch.rfft is gone); 3e-7 from the float64 operator.
#include <type_traits>

#include "ee_common.hpp"
#include "ee_square.hpp"

namespace {

using namespace ee;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 64;           // columns per staged strip
constexpr int SS = KC + 4;       // strip row stride: bank = (4 i + g + 4 s) % 64, conflict-free A-fragment reads
constexpr int STRIP = 16 * SS;   // floats per wave
constexpr int NARROW_MAX = 256;  // narrow class: largest H, W (16 bands, one per wavefront)
constexpr int WIDE_MAX = 320;    // wide class: largest H, W (20 bands, 10 wavefronts)
constexpr int WIDE_BPW = 2;      // wide class: bands per wavefront

struct BandDims {
    int H, W, HP, WP, NB, WT;  // NB = HP / 16 bands, WT = WP / 16
    int C;
};

// One wavefront's traffic between a plane and its [16][SS] LDS strip, 64 columns of a 16-row band at a time: lane l moves four
// floats of rows (l >> 4) + 4 q, q = 0 .. 3, so 16 lanes cover 256 B of one row.
template <int SQ>
struct BandIO {
    const float *src;         // the plane read
    float *dst;               // the plane written
    const float *sq_x;        // SQ == 2: the plane Add_Square's derivative is taken at
    const float *stripe_row;  // SQ != 0: this plane's stripe signs
    float *strip;
    int H, W, c, lane;
    bool vec, vec_out;
    SquareArgs sq;
    SquarePlane pl;

    __device__ __forceinline__ BandIO(const float *in, float *out, const float *sq_x_, const SquareArgs &sq_, int plane, int C, int H_, int W_,
                                      float *strip_, int lane_)
        : strip(strip_), H(H_), W(W_), c(plane % C), lane(lane_), sq(sq_), pl{} {
        const size_t poff = static_cast<size_t>(plane) * H * W;
        src = in + poff;
        dst = out + poff;
        sq_x = SQ == 2 ? sq_x_ + poff : nullptr;
        stripe_row = nullptr;
        if (SQ != 0) {
            pl = square_plane(sq, c);
            stripe_row = sq.stripe + static_cast<size_t>(plane) * W;
        }
        vec = ((W & 3) == 0) && ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) && (SQ == 0 || ((reinterpret_cast<uintptr_t>(stripe_row) & 15u) == 0));
        vec_out = ((W & 3) == 0) && ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) &&
                  (SQ != 2 || (((reinterpret_cast<uintptr_t>(sq_x) | reinterpret_cast<uintptr_t>(stripe_row)) & 15u) == 0));
    }

    __device__ __forceinline__ void load(int row0, int col0, float4 (&v)[4]) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (lane >> 4) + 4 * q, w0 = col0 + 4 * (lane & 15);
            const int h = row0 + r;
            const int hc = h < H ? h : H - 1;
            if (vec) {
                const int wc = w0 + 3 < W ? w0 : (W - 4 > 0 ? W - 4 : 0);
                v[q] = *reinterpret_cast<const float4 *>(src + static_cast<size_t>(hc) * W + wc);
            } else {
                float t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k] = src[static_cast<size_t>(hc) * W + (w0 + k < W ? w0 + k : W - 1)];
                v[q] = make_float4(t[0], t[1], t[2], t[3]);
            }
        }
    }

    __device__ __forceinline__ void stage(int row0, int col0, const float4 (&v)[4]) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (lane >> 4) + 4 * q, w0 = col0 + 4 * (lane & 15);
            const int h = row0 + r;
            float t[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int w = w0 + k;
                const bool inside = h < H && w < W;
                if (SQ == 1 && inside) {
                    float dd;
                    t[k] = square_elem<false>(sq, pl, t[k], stripe_row[w], c, h, w, dd);
                }
                if (!inside) t[k] = 0.0f;  // padding rows / columns (and the clamped loads that stood in for them)
            }
            *reinterpret_cast<float4 *>(strip + r * SS + 4 * (lane & 15)) = make_float4(t[0], t[1], t[2], t[3]);
        }
    }

    // the strip holds columns col0 .. col0 + 63 of the result band
    __device__ __forceinline__ void store(int row0, int col0) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (lane >> 4) + 4 * q, w0 = col0 + 4 * (lane & 15);
            const int h = row0 + r;
            if (h < H && w0 < W) {
                const float4 t = *reinterpret_cast<const float4 *>(strip + r * SS + 4 * (lane & 15));
                float o[4] = {t.x, t.y, t.z, t.w};
                if (SQ == 2) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (w0 + k < W) {
                            float dd = 0.0f;
                            (void)square_elem<true>(sq, pl, sq_x[static_cast<size_t>(h) * W + w0 + k], stripe_row[w0 + k], c, h, w0 + k, dd);
                            o[k] = o[k] * dd;
                        }
                }
                if (vec_out && w0 + 3 < W) {
                    *reinterpret_cast<float4 *>(dst + static_cast<size_t>(h) * W + w0) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
                    for (int k = 0; k < 4 && w0 + k < W; ++k) dst[static_cast<size_t>(h) * W + w0 + k] = o[k];
                }
            }
        }
    }
};

// blockDim.x = 64 * ceil(NB / BPW), wavefront w owns bands BPW w .. BPW w + BPW - 1 (the last wavefront may own fewer).
// MT2 = 2 nu_pad / 16 row tiles of R, NT = 2 nv_pad / 16 column tiles of [P | Q]; the tiles of R, EF are indexed [mt][nt], flat
// mt * NT + nt.  LDS: strips NW * STRIP | T1, later T4: WP * NT * 16 | rsum: MT2 * NT * 256 floats (256 x 256, MT2 = 4, NT = 2:
// 110592 B; 320 x 320, MT2 = 6, NT = 4: 150016 B).
template <int SQ, int MT2, int NT, int BPW>
__global__ __launch_bounds__(BPW == 1 ? 1024 : 64 * (WIDE_MAX / 16 / BPW)) void hfs_band_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                                                const float *__restrict__ tables, BandDims d,
                                                                                                const float *__restrict__ sq_x, SquareArgs sq) {
    static_assert(BPW != 1 || NT == 2, "one band per wavefront is the 256 x 256 class: [P | Q] 32 columns wide");
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int WP = d.WP, NB = d.NB, NW = (NB + BPW - 1) / BPW, NTHR = NW * 64;
    float *strip = lds + wave * STRIP;        // this wave's [16][SS] staging strip (later: partial R tiles, output tiles)
    float *tab = lds + NW * STRIP;            // T1, later T4: WP * NT * 16 floats
    float *rsum = tab + WP * NT * 16;         // [MT2][NT][4][64] R summed over the bands
    const int n1 = WP / 4 * NT, n2 = NB * MT2 * 4, n3 = n2;  // fragments of T1, T2, T3
    const float *g1 = tables, *g2 = g1 + n1 * 64, *g3 = g2 + n2 * 64, *g4 = g3 + n3 * 64;
    const BandIO<SQ> io(in, out, sq_x, sq, blockIdx.x, d.C, d.H, d.W, strip, lane);
    const auto mine = [NB](int band) { return BPW == 1 || band < NB; };  // wave-uniform; one band per wavefront: every wavefront has its band

    // ---- T1 -> LDS ----------------------------------------------------------------------------------------------------------
    for (int i = tid; i < WP * NT * 4; i += NTHR) reinterpret_cast<float4 *>(tab)[i] = reinterpret_cast<const float4 *>(g1)[i];
    __syncthreads();

    // ---- S1: [P | Q] of each of this wave's bands, one band after the other through the one strip ---------------------------------
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 pq[BPW][NT];
#pragma unroll
    for (int k = 0; k < BPW; ++k) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) pq[k][nt] = zero;
        const int band = wave * BPW + k, row0 = 16 * band;
        if (mine(band)) {
            float4 cur[4], nxt[4];
            io.load(row0, 0, cur);
            for (int col0 = 0; col0 < WP; col0 += KC) {
                if (col0 + KC < WP) io.load(row0, col0 + KC, nxt);  // in flight while this strip is multiplied
                io.stage(row0, col0, cur);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int ksteps = (WP - col0 < KC ? WP - col0 : KC) / 4;
                for (int s = 0; s < ksteps; ++s) {
                    const float a = strip[li * SS + 4 * s + lg];
                    const float *t1 = tab + ((col0 >> 2) + s) * NT * 64 + lane;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) pq[k][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, t1[nt * 64], pq[k][nt], 0, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();  // every lane has read the strip before it is overwritten
#pragma unroll
                for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
            }
        }
    }

    // ---- S2: this wave's share of R = CS^T [P | Q]: its bands accumulate into the same tiles, in band order -------------------------
    f32x4 rc[MT2][NT];
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) rc[mt][nt] = zero;
#pragma unroll
    for (int k = 0; k < BPW; ++k) {
        const int band = wave * BPW + k;
        if (mine(band)) {
            const float *t2 = g2 + static_cast<size_t>(band) * MT2 * 4 * 64 + lane;
#pragma unroll
            for (int mt = 0; mt < MT2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a = t2[(mt * 4 + r) * 64];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) rc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pq[k][nt][r], rc[mt][nt], 0, 0, 0);
                }
        }
    }
    __syncthreads();  // every wave is done with T1 and with its strip

    // ---- reduction of R over the waves through the strips, four tiles (1024 of a strip's 1088 floats) a round; T4 takes T1's place ------
    for (int i = tid; i < WP * NT * 4; i += NTHR) reinterpret_cast<float4 *>(tab)[i] = reinterpret_cast<const float4 *>(g4)[i];
    static_assert((MT2 * NT) % 4 == 0 && 4 * 256 <= STRIP, "four R tiles per round");
#pragma unroll
    for (int q = 0; q < MT2 * NT / 4; ++q) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) strip[(k * 4 + r) * 64 + lane] = rc[(4 * q + k) / NT][(4 * q + k) % NT][r];
        __syncthreads();
        for (int e = tid; e < 1024; e += NTHR) {
            float acc = 0.0f;
            for (int w = 0; w < NW; ++w) acc += lds[w * STRIP + e];  // wave order = band order: reproducible
            rsum[q * 1024 + e] = acc;                                 // tile 4 q + (e >> 8) = mt * NT + nt
        }
        __syncthreads();
    }

    // ---- EF (tile-wise; P tiles nt < NT / 2, Q tiles above), then S3 and S4 band by band -----------------------------------------------
    constexpr int HALF = MT2 / 2, NH = NT / 2;
    f32x4 ef[MT2][NT];
#pragma unroll
    for (int j = 0; j < HALF; ++j)
#pragma unroll
        for (int p = 0; p < NH; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = rsum[((j * NT + p) * 4 + r) * 64 + lane], cq = rsum[((j * NT + NH + p) * 4 + r) * 64 + lane];
                const float b = rsum[(((HALF + j) * NT + p) * 4 + r) * 64 + lane], dq = rsum[(((HALF + j) * NT + NH + p) * 4 + r) * 64 + lane];
                ef[j][p][r] = a - dq;
                ef[j][NH + p][r] = cq + b;
                ef[HALF + j][p][r] = b + cq;
                ef[HALF + j][NH + p][r] = dq - a;
            }
#pragma unroll
    for (int k = 0; k < BPW; ++k) {
        const int band = wave * BPW + k, row0 = 16 * band;
        if (!mine(band)) break;
        f32x4 uv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) uv[nt] = zero;
        const float *t3 = g3 + static_cast<size_t>(band) * MT2 * 4 * 64 + lane;
#pragma unroll
        for (int kt = 0; kt < MT2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float b = t3[(kt * 4 + r) * 64];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) uv[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ef[kt][nt][r], b, uv[nt], 0, 0, 0);
            }
        for (int wt0 = 0; wt0 < d.WT; wt0 += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int wt = wt0 + q;
                if (wt < d.WT) {
                    f32x4 y = zero;
                    const float *t4 = tab + wt * NT * 4 * 64 + lane;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) y = __builtin_amdgcn_mfma_f32_16x16x4f32(uv[nt][r], t4[(nt * 4 + r) * 64], y, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) strip[(4 * lg + r) * SS + 16 * q + li] = y[r];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            io.store(row0, 16 * wt0);
            __builtin_amdgcn_wave_barrier();
        }
    }
}

int table_floats(int H, int W, int nu_pad, int nv_pad) {
    const int hp = (H + 15) / 16 * 16, wp = (W + 15) / 16 * 16, mt2 = 2 * nu_pad / 16, nt = 2 * nv_pad / 16;
    return (wp / 4 * nt + 2 * (hp / 16) * mt2 * 4 + (wp / 16) * nt * 4) * 64;
}

bool narrow_pads(int nu_pad) { return nu_pad == 16 || nu_pad == 32; }
bool wide_pads(int nu_pad, int nv_pad) { return (nu_pad == 16 || nu_pad == 32 || nu_pad == 48) && (nv_pad == 16 || nv_pad == 32); }

// f(V) with the one of V... that equals v as a constant: in a generic lambda, `kernel<decltype(V)::value>` names the instantiation
template <int... V, class F>
void with_constant(int v, F f) {
    (void)((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}

// One plane class: sides up to `limit`, BPW bands per wavefront, pads_ok = (nu_pad, nv_pad) is one of the class's table widths.  The
// two entry points differ in how they report a pad outside the set: the wide one as a shape error, ahead of the size limit, the
// narrow one as unsupported, along with it.
template <int BPW>
int launch(const float *in, float *out, int B, int C, int H, int W, const float *tables, int limit, bool pads_ok, int nu_pad, int nv_pad,
           int sq_mode, const float *sq_x, float eps, const float *stripe, const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size,
           int nq, void *stream) {
    if (B < 0 || C < 1 || H < 1 || W < 1 || sq_mode < 0 || sq_mode > 2 || nq < 0 || (BPW != 1 && !pads_ok)) return EE_ERR_SHAPE;
    if (H > limit || W > limit || !pads_ok) return EE_ERR_UNSUPPORTED;
    if (B == 0) return EE_OK;
    if (!in || !out || !tables) return EE_ERR_NULL;
    if (sq_mode != 0 && (!stripe || (nq > 0 && (!sq_sign || !sq_pos || !sq_size)))) return EE_ERR_NULL;
    if (sq_mode == 2 && !sq_x) return EE_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(tables) & 15u) return EE_ERR_ALIGN;
    BandDims d{H, W, (H + 15) / 16 * 16, (W + 15) / 16 * 16, 0, 0, C};
    d.NB = d.HP / 16;
    d.WT = d.WP / 16;
    const int mt2 = 2 * nu_pad / 16, nt = 2 * nv_pad / 16, nw = (d.NB + BPW - 1) / BPW;
    const size_t lds_bytes =
        sizeof(float) * (static_cast<size_t>(nw) * STRIP + static_cast<size_t>(d.WP) * nt * 16 + static_cast<size_t>(mt2) * nt * 256);
    SquareArgs sq{stripe, sq_sign, sq_pos, sq_size, nq, C, H, W, eps, static_cast<float>(2.0 * static_cast<double>(eps))};
    const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(B) * C)), block(static_cast<unsigned>(nw * 64));
    hipStream_t st = as_stream(stream);
    ProfScope prof(sq_mode == 0 ? EE_K_HFS : (sq_mode == 1 ? EE_K_HFS_SQ_FWD : EE_K_HFS_SQ_BWD), st);
    with_constant<0, 1, 2>(sq_mode, [&](auto SQ) {
        with_constant<2, 4, 6>(mt2, [&](auto MT2) {
            with_constant<2, 4>(nt, [&](auto NT) {
                constexpr int sq_c = decltype(SQ)::value, mt2_c = decltype(MT2)::value, nt_c = decltype(NT)::value;
                if constexpr (BPW != 1 || (mt2_c <= 4 && nt_c == 2)) {  // the narrow class has no wider tables
                    const auto kernel = hfs_band_kernel<sq_c, mt2_c, nt_c, BPW>;
                    static bool opted = false;  // per instantiation
                    if (!opted && lds_bytes > 64 * 1024) {
                        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
                            hipSuccess)
                            (void)hipGetLastError();
                        opted = true;
                    }
                    EE_LAUNCH(kernel, grid, block, lds_bytes, st, in, out, tables, d, sq_x, sq);
                }
            });
        });
    });
    return launch_status();
}

}  // namespace

EE_API int ee_hfs_mfma_table_floats(int H, int W, int nu_pad) {
    if (H < 1 || W < 1 || H > NARROW_MAX || W > NARROW_MAX || !narrow_pads(nu_pad)) return EE_ERR_SHAPE;
    return table_floats(H, W, nu_pad, 16);
}

EE_API int ee_hfs_mfma_f32(const float *in, float *out, int B, int C, int H, int W, const float *tables, int nu_pad, int sq_mode,
                           const float *sq_x, float eps, const float *stripe, const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size,
                           int nq, void *stream) {
    return launch<1>(in, out, B, C, H, W, tables, NARROW_MAX, narrow_pads(nu_pad), nu_pad, 16, sq_mode, sq_x, eps, stripe, sq_sign, sq_pos,
                     sq_size, nq, stream);
}

EE_API int ee_hfs_wide_table_floats(int H, int W, int nu_pad, int nv_pad) {
    if (H < 1 || W < 1 || !wide_pads(nu_pad, nv_pad)) return EE_ERR_SHAPE;
    if (H > WIDE_MAX || W > WIDE_MAX) return EE_ERR_UNSUPPORTED;
    return table_floats(H, W, nu_pad, nv_pad);
}

EE_API int ee_hfs_wide_f32(const float *in, float *out, int B, int C, int H, int W, const float *tables, int nu_pad, int nv_pad, int sq_mode,
                           const float *sq_x, float eps, const float *stripe, const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size,
                           int nq, void *stream) {
    return launch<WIDE_BPW>(in, out, B, C, H, W, tables, WIDE_MAX, wide_pads(nu_pad, nv_pad), nu_pad, nv_pad, sq_mode, sq_x, eps, stripe, sq_sign,
                            sq_pos, sq_size, nq, stream);
}

