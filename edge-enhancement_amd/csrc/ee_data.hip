// ee_data.hip - batch assembly from a device-resident uint8 dataset split (gfx950).
//
// One launch per batch: gather the batch's samples from the split [N,H,W,C] u8, mirror the flagged ones along W,
// convert u8 -> f32 through a 256-entry table (lut[v] = float(v) / 255, built by the caller with torch's own division, so
// the values are ToTensor's bit for bit) and transpose HWC -> NCHW; the labels of the batch are gathered in the same launch.
// HBM-bound and launch-bound: 4 bytes read per 16 bytes written (C = 1: 1 per 16 B).
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
