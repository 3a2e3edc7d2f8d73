// ee_data.hip - batch assembly from a device-resident uint8 dataset split (gfx950).
//
// One launch per batch: gather the batch's samples from the split [N,H,W,C] u8, mirror the flagged ones along W,
// convert u8 -> f32 through a 256-entry table (lut[v] = float(v) / 255, built by the caller with torch's own division, so
// the values are ToTensor's bit for bit) and transpose HWC -> NCHW; the labels of the batch are gathered in the same launch.
// HBM-bound and launch-bound: 4 bytes read per 16 bytes written (C = 1: 1 per 16 B).
//
// ee_batch_rrc_u8_f32 does the same for a split of images of different sizes (ImageNet train): each sample's crop box is
// resampled to S x S with PIL's 8-bit BILINEAR arithmetic (coefficients formed in double, 22-bit fixed point, a horizontal pass
// to uint8 and a vertical pass over that), so a batch is ToTensor(resize(crop(img))) bit for bit.
#include "ee_common.hpp"

namespace {

using namespace ee;

__device__ __forceinline__ float nanf_() { return __int_as_float(0x7fc00000); }

// VEC: each thread writes 4 consecutive outputs of one (b, c, h) row with one 16-byte store and reads its 4 source pixels as
// aligned dwords (W % 4 == 0, so a group of 4 columns starts at a multiple of 4 pixels - also when mirrored - and covers
// 4*C bytes at a 4-byte aligned offset: 1 dword for C = 1, 3 dwords for C = 3).  !VEC: one output per thread, byte loads.
// Thread t owns output float4 t (VEC) or float t: the grid follows the layout of `out`, so the stores are fully coalesced.
template <bool VEC, int C>
__global__ __launch_bounds__(kBlock) void batch_u8_kernel(const uint8_t *__restrict__ data, const int64_t *__restrict__ labels,
                                                          const int32_t *__restrict__ idx, const uint8_t *__restrict__ flip,
                                                          const float *__restrict__ lut, int64_t N, int B, int H, int W,
                                                          float *__restrict__ out, int64_t *__restrict__ labels_out) {
    __shared__ float s_lut[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = lut[i];
    __syncthreads();

    const int64_t tid0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t b = tid0; b < B; b += stride) {
        const int64_t s = idx[b];
        labels_out[b] = (s >= 0 && s < N) ? labels[s] : -1;
    }
    const int Wg = VEC ? W / 4 : W;  // work items per output row
    const int64_t total = static_cast<int64_t>(B) * C * H * Wg;
    for (int64_t t = tid0; t < total; t += stride) {
        int64_t r = t;
        const int q = static_cast<int>(r % Wg);
        r /= Wg;
        const int h = static_cast<int>(r % H);
        r /= H;
        const int c = static_cast<int>(r % C);
        const int b = static_cast<int>(r / C);
        const int64_t s = idx[b];
        if (s < 0 || s >= N) {  // outside the documented precondition: never read out of bounds, make the batch visibly wrong
            if (VEC)
                reinterpret_cast<float4 *>(out)[t] = make_float4(nanf_(), nanf_(), nanf_(), nanf_());
            else
                out[t] = nanf_();
            continue;
        }
        const bool f = flip != nullptr && flip[s] != 0;
        const uint8_t *row = data + (s * H + h) * static_cast<int64_t>(W) * C;
        if (VEC) {
            const int w0 = f ? W - 4 - 4 * q : 4 * q;  // first source column of the group
            const uint32_t *src = reinterpret_cast<const uint32_t *>(row + static_cast<int64_t>(w0) * C);
            uint32_t v[4];  // the byte of channel c of source columns w0 .. w0+3
            if (C == 1) {
                const uint32_t d = src[0];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (d >> (8 * k)) & 0xffu;
            } else {
                const uint32_t d0 = src[0], d1 = src[1], d2 = src[2];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int byte = 3 * k + c;  // 0 .. 11 across d0 d1 d2
                    const uint32_t d = byte < 4 ? d0 : (byte < 8 ? d1 : d2);
                    v[k] = (d >> (8 * (byte & 3))) & 0xffu;
                }
            }
            float4 o;
            if (f) {
                o.x = s_lut[v[3]], o.y = s_lut[v[2]], o.z = s_lut[v[1]], o.w = s_lut[v[0]];
            } else {
                o.x = s_lut[v[0]], o.y = s_lut[v[1]], o.z = s_lut[v[2]], o.w = s_lut[v[3]];
            }
            reinterpret_cast<float4 *>(out)[t] = o;
        } else {
            const int w = f ? W - 1 - q : q;
            out[t] = s_lut[row[static_cast<int64_t>(w) * C + c]];
        }
    }
}

template <bool VEC>
void launch(int C, const uint8_t *data, const int64_t *labels, const int32_t *idx, const uint8_t *flip, const float *lut, int64_t N,
            int B, int H, int W, float *out, int64_t *labels_out, hipStream_t st) {
    const int64_t work = static_cast<int64_t>(B) * C * H * (VEC ? W / 4 : W);
    int64_t blocks = (work + kBlock - 1) / kBlock;
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    const dim3 grid(static_cast<unsigned>(blocks));
    if (C == 1)
        EE_LAUNCH((batch_u8_kernel<VEC, 1>), grid, dim3(kBlock), 0, st, data, labels, idx, flip, lut, N, B, H, W, out, labels_out);
    else
        EE_LAUNCH((batch_u8_kernel<VEC, 3>), grid, dim3(kBlock), 0, st, data, labels, idx, flip, lut, N, B, H, W, out, labels_out);
}

// ---- crop + PIL BILINEAR resample to S x S (RandomResizedCrop) -----------------------------------------------------------------
// One axis of PIL's ImagingResample (precompute_coeffs + normalize_coeffs_8bpc) for `in` source and `out` result pixels:
// result pixel xx reads the n source pixels from xmin on, tap x with weight max(0, 1 - |(x + xmin - center + 0.5) / fs|) over
// their sum ww (summed in ascending x), as the integer (int)(0.5 + w / ww * 2^22).  All of it in double, in the operation order of
// eeadv.data.resample_coeffs (the file is built without contraction and fast-math).  One step is not PIL's own: PIL multiplies the
// filter argument by ss = 1.0 / filterscale, here and in the restatement it is divided by fs.  The 22-bit integers of the two forms
// were compared for in = 1..1199, out in {24, 43, 224} without a difference, and the tests hold the restatement against PIL.
constexpr int kPrec = 22;
constexpr int kBand = 16;          // result rows of one workgroup
constexpr int kStageWords = 10240;  // 40 KB of LDS for the coefficient tables and the horizontally resampled source rows

struct Axis {
    double scale, fs;
    int in, ksize;
};
__device__ __forceinline__ Axis make_axis(int in, int out) {
    Axis a;
    a.in = in;
    a.scale = static_cast<double>(in) / static_cast<double>(out);
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    const double k = ceil(a.fs) * 2.0 + 1.0;
    a.ksize = k < 1.0e9 ? static_cast<int>(k) : 1000000000;  // only sizes the LDS tables: anything this large takes the direct path
    return a;
}
__device__ __forceinline__ double tap_weight(const Axis &a, double center, int xmin, int x) {
    const double t = fabs((static_cast<double>(x + xmin) - center + 0.5) / a.fs);
    return t < 1.0 ? 1.0 - t : 0.0;
}
// window of result pixel xx: first source pixel, number of taps, the centre and the sum of the weights
__device__ __forceinline__ void axis_window(const Axis &a, int xx, int &xmin, int &n, double &center, double &ww) {
    center = (static_cast<double>(xx) + 0.5) * a.scale;
    xmin = static_cast<int>(center - a.fs + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = static_cast<int>(center + a.fs + 0.5);
    if (xmax > a.in) xmax = a.in;
    n = xmax - xmin;
    ww = 0.0;
    for (int x = 0; x < n; ++x) ww += tap_weight(a, center, xmin, x);
}
__device__ __forceinline__ int tap_coef(const Axis &a, double center, int xmin, int x, double ww) {
    double w = tap_weight(a, center, xmin, x);
    if (ww != 0.0) w /= ww;
    return static_cast<int>(0.5 + w * static_cast<double>(1 << kPrec));
}
__device__ __forceinline__ uint32_t clip8(int acc) {
    const int v = acc >> kPrec;
    return static_cast<uint32_t>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Workgroup (b, band): the kBand result rows from band * kBand on of sample idx[b], all 3 channels.
// Staged path: the coefficient tables of the S columns and of the band's rows go to LDS once; then, for as many consecutive
// result rows as fit (at least one), the source rows they need are resampled horizontally into LDS as uint8 - planar, each row
// padded to a multiple of 4 bytes, already mirrored when the sample is flagged - and the vertical pass reads them as aligned dwords
// and writes 4 consecutive floats of one (c, row) per thread (one 16-byte store when VEC).  Direct path, for a crop so large
// against S that the tables or one row's window do not fit: one thread per output forms every coefficient itself and reads the
// crop from global memory (same integers, slow; at S = 224 a crop of more than about 2400 pixels on a side).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void batch_rrc_kernel(const uint8_t *__restrict__ pixels, int64_t nbytes,
                                                           const int64_t *__restrict__ offsets, const int32_t *__restrict__ sizes,
                                                           const int64_t *__restrict__ labels, const int32_t *__restrict__ idx,
                                                           const int32_t *__restrict__ boxes, const uint8_t *__restrict__ flip,
                                                           const float *__restrict__ lut, int64_t N, int S, int nbands,
                                                           float *__restrict__ out, int64_t *__restrict__ labels_out) {
    __shared__ float s_lut[256];
    __shared__ uint32_t s_stage[kStageWords];
    __shared__ int s_ymin[kBand], s_yn[kBand];

    const int tid = threadIdx.x;
    const int b = static_cast<int>(blockIdx.x) / nbands, band = static_cast<int>(blockIdx.x) - b * nbands;
    const int r0 = band * kBand, r1 = min(S, r0 + kBand), nr = r1 - r0;
    const int64_t s = idx[b];
    float *const outb = out + static_cast<int64_t>(b) * 3 * S * S;
    const int Q = (S + 3) / 4;  // groups of 4 columns per row

    // the sample, its image and its box: anything outside the preconditions is never read and gives NaN / -1
    bool ok = s >= 0 && s < N;
    int H = 0, W = 0, top = 0, left = 0, h = 0, w = 0;
    int64_t off = 0;
    if (ok) {
        H = sizes[2 * s], W = sizes[2 * s + 1];
        top = boxes[4 * s], left = boxes[4 * s + 1], h = boxes[4 * s + 2], w = boxes[4 * s + 3];
        off = offsets[s];
        ok = H >= 1 && W >= 1 && off >= 0 && off <= nbytes && static_cast<int64_t>(H) * W * 3 <= nbytes - off && top >= 0 && left >= 0 &&
             h >= 1 && w >= 1 && static_cast<int64_t>(top) + h <= H && static_cast<int64_t>(left) + w <= W;
    }
    if (band == 0 && tid == 0) labels_out[b] = ok ? labels[s] : -1;
    if (!ok) {
        for (int t = tid; t < 3 * nr * S; t += kBlock) {
            const int c = t / (nr * S), r = (t - c * nr * S) / S, x = t - (c * nr + r) * S;
            outb[(static_cast<int64_t>(c) * S + r0 + r) * S + x] = nanf_();
        }
        return;
    }
    const bool f = flip != nullptr && flip[s] != 0;
    const uint8_t *const img = pixels + off + (static_cast<int64_t>(top) * W + left) * 3;  // the crop's first byte; row pitch W * 3
    const int64_t pitch = static_cast<int64_t>(W) * 3;
    const Axis ax = make_axis(w, S), ay = make_axis(h, S);

    for (int i = tid; i < 256; i += kBlock) s_lut[i] = lut[i];

    // LDS plan (words): kx [S * ksize_x] | ky [kBand * ksize_y] | xmin [S] | xn [S] | rows: 3 planes of rowcap rows of P bytes
    const int P = Q * 4;
    const int64_t table_words = static_cast<int64_t>(S) * ax.ksize + static_cast<int64_t>(kBand) * ay.ksize + 2 * static_cast<int64_t>(S);
    const int64_t rowcap64 = table_words < kStageWords ? (kStageWords - table_words) * 4 / (3 * static_cast<int64_t>(P)) : 0;
    if (rowcap64 < ay.ksize) {  // direct path
        __syncthreads();
        for (int t = tid; t < 3 * nr * S; t += kBlock) {
            const int c = t / (nr * S), r = (t - c * nr * S) / S, x = t - (c * nr + r) * S;
            const int xx = f ? S - 1 - x : x;
            int xmin, xn, ymin, yn;
            double xc, xww, yc, yww;
            axis_window(ax, xx, xmin, xn, xc, xww);
            axis_window(ay, r0 + r, ymin, yn, yc, yww);
            int acc = 1 << (kPrec - 1);
            for (int y = 0; y < yn; ++y) {
                const uint8_t *src = img + (ymin + y) * pitch + static_cast<int64_t>(xmin) * 3 + c;
                int hacc = 1 << (kPrec - 1);
                for (int k = 0; k < xn; ++k) hacc += static_cast<int>(src[3 * k]) * tap_coef(ax, xc, xmin, k, xww);
                acc += static_cast<int>(clip8(hacc)) * tap_coef(ay, yc, ymin, y, yww);
            }
            outb[(static_cast<int64_t>(c) * S + r0 + r) * S + x] = s_lut[clip8(acc)];
        }
        return;
    }
    const int rowcap = static_cast<int>(rowcap64 < (1 << 20) ? rowcap64 : (1 << 20));
    int *const s_kx = reinterpret_cast<int *>(s_stage);
    int *const s_ky = s_kx + S * ax.ksize;
    int *const s_xmin = s_ky + kBand * ay.ksize;
    int *const s_xn = s_xmin + S;
    uint8_t *const s_rows = reinterpret_cast<uint8_t *>(s_xn + S);

    for (int i = tid; i < S + nr; i += kBlock) {
        const bool col = i < S;
        const Axis &a = col ? ax : ay;
        const int xx = col ? i : r0 + (i - S);
        int xmin, n;
        double center, ww;
        axis_window(a, xx, xmin, n, center, ww);
        int *const k = col ? s_kx + i * ax.ksize : s_ky + (i - S) * ay.ksize;
        for (int x = 0; x < n; ++x) k[x] = tap_coef(a, center, xmin, x, ww);
        if (col)
            s_xmin[i] = xmin, s_xn[i] = n;
        else
            s_ymin[i - S] = xmin, s_yn[i - S] = n;
    }
    __syncthreads();

    for (int ra = 0; ra < nr;) {  // result rows [ra, rb) of the band share one stage of source rows [base, base + rows)
        const int base = s_ymin[ra];
        int rb = ra + 1;
        while (rb < nr && s_ymin[rb] + s_yn[rb] - base <= rowcap) ++rb;
        const int rows = s_ymin[rb - 1] + s_yn[rb - 1] - base;
        // horizontal pass: item (source row j, result column xx), the 3 channels of one pixel
        for (int t = tid; t < rows * S; t += kBlock) {
            const int j = t / S, xx = t - j * S;
            const int n = s_xn[xx];
            const int *const k = s_kx + xx * ax.ksize;
            const uint8_t *src = img + (base + j) * pitch + static_cast<int64_t>(s_xmin[xx]) * 3;
            int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < n; ++x) {
                const int kk = k[x];
                a0 += static_cast<int>(src[3 * x]) * kk;
                a1 += static_cast<int>(src[3 * x + 1]) * kk;
                a2 += static_cast<int>(src[3 * x + 2]) * kk;
            }
            const int xo = f ? S - 1 - xx : xx;
            s_rows[(0 * rowcap + j) * P + xo] = static_cast<uint8_t>(clip8(a0));
            s_rows[(1 * rowcap + j) * P + xo] = static_cast<uint8_t>(clip8(a1));
            s_rows[(2 * rowcap + j) * P + xo] = static_cast<uint8_t>(clip8(a2));
        }
        __syncthreads();
        // vertical pass: item (c, result row r, group q of 4 columns)
        const int nrow = rb - ra;
        for (int t = tid; t < 3 * nrow * Q; t += kBlock) {
            const int c = t / (nrow * Q), r = ra + (t - c * nrow * Q) / Q, q = t - (c * nrow + (r - ra)) * Q;
            const int n = s_yn[r];
            const int *const k = s_ky + r * ay.ksize;
            const uint32_t *src = reinterpret_cast<const uint32_t *>(s_rows + (c * rowcap + (s_ymin[r] - base)) * P) + q;
            int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int y = 0; y < n; ++y) {
                const uint32_t d = src[y * Q];
                const int kk = k[y];
                a0 += static_cast<int>(d & 0xffu) * kk;
                a1 += static_cast<int>((d >> 8) & 0xffu) * kk;
                a2 += static_cast<int>((d >> 16) & 0xffu) * kk;
                a3 += static_cast<int>(d >> 24) * kk;
            }
            float *const dst = outb + (static_cast<int64_t>(c) * S + r0 + r) * S + 4 * q;
            const float o0 = s_lut[clip8(a0)], o1 = s_lut[clip8(a1)], o2 = s_lut[clip8(a2)], o3 = s_lut[clip8(a3)];
            if (VEC) {
                *reinterpret_cast<float4 *>(dst) = make_float4(o0, o1, o2, o3);
            } else {  // S % 4 != 0: the last group of a row is partial (its padding bytes in LDS are never meaningful)
                const int left4 = S - 4 * q;
                dst[0] = o0;
                if (left4 > 1) dst[1] = o1;
                if (left4 > 2) dst[2] = o2;
                if (left4 > 3) dst[3] = o3;
            }
        }
        __syncthreads();
        ra = rb;
    }
}

// ---- crop from the zero-padded image + mirror + NEAREST rotation (RandomCrop + RandomHorizontalFlip + RandomRotation) -----------
// Thread t owns output float4 t (VEC: W % 4 == 0) or float t of out [B,C,H,W].  Output pixel (x, y) of sample b reads pixel
// (xin, yin) = ((a2 + x a0 + y a1) >> 16, (a5 + x a3 + y a4) >> 16) of the rotation's source, the mirrored crop; outside its W x H
// frame it is the fill.  Column xin of the mirrored crop is column W-1-xin of the crop, and crop pixel (xs, yin) is image pixel
// (xs + left - pad, yin + top - pad), 0 outside the image.  64-bit products: no (H, W, coefficient) can overflow them.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void batch_aug_kernel(const uint8_t *__restrict__ data, const int64_t *__restrict__ labels,
                                                           const int32_t *__restrict__ idx, const int32_t *__restrict__ offs,
                                                           const uint8_t *__restrict__ flip, const int32_t *__restrict__ coef,
                                                           const float *__restrict__ lut, int64_t N, int B, int C, int H, int W, int pad,
                                                           float *__restrict__ out, int64_t *__restrict__ labels_out) {
    __shared__ float s_lut[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = lut[i];
    __syncthreads();

    const int64_t tid0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t b = tid0; b < B; b += stride) {
        const int64_t s = idx[b];
        const int top = offs[2 * b], left = offs[2 * b + 1];
        labels_out[b] = (s >= 0 && s < N && top >= 0 && top <= 2 * pad && left >= 0 && left <= 2 * pad) ? labels[s] : -1;
    }
    constexpr int K = VEC ? 4 : 1;
    const int Wg = W / K;  // work items per output row
    const int64_t total = static_cast<int64_t>(B) * C * H * Wg;
    for (int64_t t = tid0; t < total; t += stride) {
        int64_t r = t;
        const int q = static_cast<int>(r % Wg);
        r /= Wg;
        const int y = static_cast<int>(r % H);
        r /= H;
        const int c = static_cast<int>(r % C);
        const int b = static_cast<int>(r / C);
        const int64_t s = idx[b];
        const int top = offs[2 * b], left = offs[2 * b + 1];
        float o[K];
        if (s < 0 || s >= N || top < 0 || top > 2 * pad || left < 0 || left > 2 * pad) {
            // outside the documented precondition: never read out of bounds, make the batch visibly wrong
#pragma unroll
            for (int k = 0; k < K; ++k) o[k] = nanf_();
        } else {
            const bool f = flip != nullptr && flip[b] != 0;
            const int32_t *const a = coef + 6 * static_cast<int64_t>(b);
            const int64_t a0 = a[0], a3 = a[3];
            const int64_t xr = a[2] + static_cast<int64_t>(y) * a[1], yr = a[5] + static_cast<int64_t>(y) * a[4];
            const uint8_t *const img = data + s * H * static_cast<int64_t>(W) * C + c;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int x = K * q + k;
                const int64_t xin = (xr + x * a0) >> 16, yin = (yr + x * a3) >> 16;
                uint32_t v = 0;  // the fill; lut[0] = 0.0f
                if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
                    const int64_t xs = (f ? W - 1 - xin : xin) + left - pad, ys = yin + top - pad;
                    if (xs >= 0 && xs < W && ys >= 0 && ys < H) v = img[(ys * W + xs) * C];
                }
                o[k] = s_lut[v];
            }
        }
        if (VEC)
            reinterpret_cast<float4 *>(out)[t] = make_float4(o[0], o[K > 1 ? 1 : 0], o[K > 2 ? 2 : 0], o[K > 3 ? 3 : 0]);
        else
            out[t] = o[0];
    }
}

}  // namespace

EE_API int ee_batch_u8_f32(const uint8_t *data, const int64_t *labels, const int32_t *idx, const uint8_t *flip, const float *lut,
                           long long N, int B, int C, int H, int W, float *out, int64_t *labels_out, void *stream) {
    if (B < 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0) return EE_ERR_SHAPE;
    if (C != 1 && C != 3) return EE_ERR_UNSUPPORTED;
    if (B == 0) return EE_OK;
    if (!data || !labels || !idx || !lut || !out || !labels_out) return EE_ERR_NULL;
    if (!aligned4(out) || !aligned4(lut) || !aligned4(idx) || (reinterpret_cast<uintptr_t>(labels) & 7u) ||
        (reinterpret_cast<uintptr_t>(labels_out) & 7u))
        return EE_ERR_ALIGN;
    const bool vec = W % 4 == 0 && aligned16(out) && aligned4(data);
    if (vec)
        launch<true>(C, data, labels, idx, flip, lut, N, B, H, W, out, labels_out, as_stream(stream));
    else
        launch<false>(C, data, labels, idx, flip, lut, N, B, H, W, out, labels_out, as_stream(stream));
    return launch_status();
}

EE_API int ee_batch_rrc_u8_f32(const uint8_t *pixels, long long nbytes, const int64_t *offsets, const int32_t *sizes, const int64_t *labels,
                               const int32_t *idx, const int32_t *boxes, const uint8_t *flip, const float *lut, long long N, int B, int S,
                               float *out, int64_t *labels_out, void *stream) {
    if (B < 0 || N <= 0 || S <= 0 || nbytes <= 0) return EE_ERR_SHAPE;
    if (S > 4096) return EE_ERR_UNSUPPORTED;
    if (B == 0) return EE_OK;
    if (!pixels || !offsets || !sizes || !labels || !idx || !boxes || !lut || !out || !labels_out) return EE_ERR_NULL;
    if (!aligned4(out) || !aligned4(lut) || !aligned4(idx) || !aligned4(sizes) || !aligned4(boxes) || (reinterpret_cast<uintptr_t>(labels) & 7u) ||
        (reinterpret_cast<uintptr_t>(offsets) & 7u) || (reinterpret_cast<uintptr_t>(labels_out) & 7u))
        return EE_ERR_ALIGN;
    const int nbands = (S + kBand - 1) / kBand;
    if (static_cast<int64_t>(B) * nbands > 0x7fffffff) return EE_ERR_UNSUPPORTED;
    const dim3 grid(static_cast<unsigned>(B) * static_cast<unsigned>(nbands));
    if (S % 4 == 0 && aligned16(out))
        EE_LAUNCH((batch_rrc_kernel<true>), grid, dim3(kBlock), 0, as_stream(stream), pixels, static_cast<int64_t>(nbytes), offsets, sizes, labels,
                  idx, boxes, flip, lut, static_cast<int64_t>(N), S, nbands, out, labels_out);
    else
        EE_LAUNCH((batch_rrc_kernel<false>), grid, dim3(kBlock), 0, as_stream(stream), pixels, static_cast<int64_t>(nbytes), offsets, sizes, labels,
                  idx, boxes, flip, lut, static_cast<int64_t>(N), S, nbands, out, labels_out);
    return launch_status();
}

EE_API int ee_batch_aug_u8_f32(const uint8_t *data, const int64_t *labels, const int32_t *idx, const int32_t *offs, const uint8_t *flip,
                               const int32_t *coef, const float *lut, const int32_t *idx_host, const int32_t *offs_host, long long N, int B, int C,
                               int H, int W, int pad, float *out, int64_t *labels_out, void *stream) {
    if (B < 0 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || pad < 0) return EE_ERR_SHAPE;
    if (pad > (1 << 20) || static_cast<int64_t>(H) * W > (int64_t(1) << 40) / C) return EE_ERR_UNSUPPORTED;
    if (B == 0) return EE_OK;
    if (!data || !labels || !idx || !offs || !coef || !lut || !idx_host || !offs_host || !out || !labels_out) return EE_ERR_NULL;
    if (!aligned4(out) || !aligned4(lut) || !aligned4(idx) || !aligned4(offs) || !aligned4(coef) || !aligned4(idx_host) || !aligned4(offs_host) ||
        (reinterpret_cast<uintptr_t>(labels) & 7u) || (reinterpret_cast<uintptr_t>(labels_out) & 7u))
        return EE_ERR_ALIGN;
    for (int b = 0; b < B; ++b) {  // the host's copy of the draws: nothing is launched on a sample or a crop outside its range
        if (idx_host[b] < 0 || idx_host[b] >= N) return EE_ERR_SHAPE;
        if (offs_host[2 * b] < 0 || offs_host[2 * b] > 2 * pad || offs_host[2 * b + 1] < 0 || offs_host[2 * b + 1] > 2 * pad) return EE_ERR_SHAPE;
    }
    const bool vec = W % 4 == 0 && aligned16(out);
    const int64_t work = static_cast<int64_t>(B) * C * H * (vec ? W / 4 : W);
    int64_t blocks = (work + kBlock - 1) / kBlock;
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    const dim3 grid(static_cast<unsigned>(blocks));
    ProfScope prof(EE_K_BATCH_AUG, as_stream(stream));
    if (vec)
        EE_LAUNCH((batch_aug_kernel<true>), grid, dim3(kBlock), 0, as_stream(stream), data, labels, idx, offs, flip, coef, lut, static_cast<int64_t>(N),
                  B, C, H, W, pad, out, labels_out);
    else
        EE_LAUNCH((batch_aug_kernel<false>), grid, dim3(kBlock), 0, as_stream(stream), data, labels, idx, offs, flip, coef, lut,
                  static_cast<int64_t>(N), B, C, H, W, pad, out, labels_out);
    return launch_status();
}
