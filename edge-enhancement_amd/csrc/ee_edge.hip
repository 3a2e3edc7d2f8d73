// ee_edge.hip - CannyFilter_step125_1 (utils/core.py:509-585) forward / backward and the fused EE front
// end, as LDS-tiled, register-blocked stencil kernels for gfx950.
//
// Tiling.  One 256-thread workgroup (4 waves) owns a TH x TW tile of one image (16x64 when W > 32, else
// 32x32); grid = B * tilesY * tilesX, e.g. 400 workgroups for a batch of 100 64x64 images.  The only data
// staged in LDS are the clamped input frame (tile + halo, filled with 16-B global loads / 16-B LDS
// stores; replicate padding = clamped coordinates, never a padded tensor) and, in the backward, the
// per-pixel magnitude gradients.  Each lane owns 4 consecutive pixels of a row: it pulls a 5x8 window per
// channel out of LDS (ds_read_b64), keeps the 3x6 blurred neighbourhood of all channels in registers and
// runs the Sobel / magnitude / threshold chain there, so the forward needs ONE barrier and the backward
// three.  All global traffic is 16 B per lane (1 KiB per wave-instruction) and is issued before the first
// barrier, so its latency hides under the stencil arithmetic.
//
// Arithmetic is identical, operation for operation, to oracle/ee_oracle.c (fmaf chains: blur row-major over
// taps, Sobel over (kh, kw, c) with c innermost; IEEE divide / sqrt; -ffp-contract=off): edge bits, gate
// bits and gradients (NaNs included) are bit-exact against the oracle.
#include <math.h>

#include "ee_common.hpp"
#include "ee_stencil.hpp"

namespace {

using namespace ee;

// =====================================================================================================
// forward:  edge map, optionally fused with  x_in = clamp(x_hfs + w*edge, 0, 1)  and the clamp gate
// =====================================================================================================
template <int C, int TH, int TW, bool FUSED>
__global__ __launch_bounds__(kBlock) void edge_fwd_kernel(EdgeParams p, Weights wt) {
    constexpr int FH = TH + 4, FW = TW + 2 * kColHalo;
    __shared__ __align__(16) float xs[C * FH * FW];
    const int H = p.H, W = p.W;
    const Lane l = lane_of<TH, TW>(p);
    const int n = l.n, i = l.ti, jb = l.tjb;
    const bool vec = p.vec != 0;

    // low-pass branch values for this lane's pixels: issued before the barrier so the latency overlaps the stencil
    float4 xh[C];
    if (FUSED) load_px4<C, false>(p.x_hfs, nullptr, n, H, W, i, jb, l.live, vec, xh, nullptr);
    load_frame<FH, FW, kColHalo, C>(xs, p.x + static_cast<size_t>(n) * C * H * W, C, H, W, l.i0, l.j0, 2, vec);
    __syncthreads();
    if (!l.live) return;

    float b[C][3][6];
    blur_group<C, FH, FW>(xs, wt, i - l.i0, jb - l.j0 + kColHalo - 2, i, jb, H, W, b);
    float e[4], m[4], gxs[4], gys[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ax, ay, s2, mag_a;
        sobel_px<C>(b, wt, k, ax, ay);
        edge_from_sums<C>(ax, ay, p.alpha, p.high, gxs[k], gys[k], s2, m[k], mag_a, e[k]);
    }
    const size_t pix = plane_at(n, 1, 0, H, W, i, jb);
    by_vec(vec, [&](auto v) {
        constexpr bool VEC = decltype(v)::value;
        if (p.edge) store_px4<VEC>(p.edge, pix, jb, W, e);
        if (p.mag) store_px4<VEC>(p.mag, pix, jb, W, m);
        if (p.gx_out) {
            store_px4<VEC>(p.gx_out, pix, jb, W, gxs);
            store_px4<VEC>(p.gy_out, pix, jb, W, gys);
        }
        if (FUSED) store_combine<C, VEC>(p.x_in, p.gate, n, H, W, i, jb, xh, e, p.w);
    });
}

// =====================================================================================================
// backward:  g_img = adjoint of the edge filter applied to u (NaN-faithful); the fused variant forms
//            g_hfs = g_in * gate and u = w * sum_c g_hfs_c itself.
//
// Frame = (TH+8) x (TW+8) positions with origin at image pixel (i0-4, j0-4).
//   stage 1 (global -> LDS/regs): clamped x frame; u on the frame; this lane's g_in / gate values
//   stage 2: gg = d(loss)/d(gx1, gy1) per pixel, rows/cols [i0-2, i0+TH+2) x [j0-2, j0+TW+2), 0 outside the image
//   stage 3: gb = ReplicationPad^T( Sx^T ggx + Sy^T ggy ), rows/cols [i0-1, i0+TH+1) x [j0-1, j0+TW+1)
//   stage 4: out = ReplicationPad^T( G^T gb ) on the tile
// Transposed correlations visit taps in row-major order as one fmaf chain and DO multiply zero-weight
// taps (0 * NaN = NaN, like a GEMM-based dgrad); the pad adjoint adds its cells in raster order.
//
// SAVED (fused only): the forward kept gx1, gy1 (8 B per pixel), so the backward neither re-reads x nor recomputes
// blur + Sobel (~60 % of the recomputing kernel's instructions): no x frame, and stage 1 puts this lane's stage-2 group
// of gx1 / gy1 straight into registers, issued first.  Same stages 2-4, same arithmetic on the same values: bit-identical.
// =====================================================================================================
template <int C, int TH, int TW, bool FUSED, bool SAVED>
__global__ __launch_bounds__(kBlock) void edge_bwd_kernel(EdgeParams p, Weights wt) {
    constexpr int FH = TH + 8, FW = TW + 2 * kColHalo, PL = FH * FW, NX = SAVED ? 0 : C;
    constexpr int GG_GX = (TW + 4 + 3) / 4, GG_ROWS = TH + 4;  // 4-pixel groups of the gg region
    static_assert(!SAVED || FUSED, "the saved responses belong to the fused front end");
    static_assert(!SAVED || GG_ROWS * GG_GX <= kBlock, "stage 2 must be one round: its operands are preloaded per lane");
    __shared__ __align__(16) float lds[(NX + 4) * PL];
    float *xs = lds;            // [NX] planes: clamped input frame (SAVED: none - xs is us and must not be read)
    float *us = lds + NX * PL;  // upstream gradient u on the frame
    float *ggx = us + PL, *ggy = ggx + PL, *gb = ggy + PL;  // zero wherever nothing is written (see stage 1)
    const int H = p.H, W = p.W;
    const Lane l = lane_of<TH, TW>(p);
    const int n = l.n, oi = l.i0 - 4, oj = l.j0 - kColHalo;  // image coordinates of frame (0, 0)
    const bool vec = p.vec != 0;

    // ---- stage 1: every global load of the kernel, issued up front ------------------------------------------------------
    float gxv[4], gyv[4];
    if (SAVED) {  // the responses of stage-2 group threadIdx.x, on clamped addresses
        const Group q = group_of<GG_GX, 2, 2>(threadIdx.x, oi, oj, H, W);
        const size_t row = plane_at(n, 1, 0, H, W, clampi(q.i, 0, H - 1), 0);
        if (vec) {  // q.jb = j0 - 2 + 4 g is even: two 8-byte loads per plane, columns clamped into the row
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const int jc = clampi(q.jb + 2 * hlf, 0, W - 2);
                const float2 a = *reinterpret_cast<const float2 *>(p.gx_in + row + jc);
                const float2 b = *reinterpret_cast<const float2 *>(p.gy_in + row + jc);
                gxv[2 * hlf] = a.x; gxv[2 * hlf + 1] = a.y;
                gyv[2 * hlf] = b.x; gyv[2 * hlf + 1] = b.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int jc = clampi(q.jb + k, 0, W - 1);
                gxv[k] = p.gx_in[row + jc];
                gyv[k] = p.gy_in[row + jc];
            }
        }
    }
    float4 gin[FUSED ? C : 1];
    uchar4 gtv[FUSED ? C : 1];
    if (FUSED) load_px4<C, true>(p.g_in, p.gate_in, n, H, W, l.ti, l.tjb, l.live, vec, gin, gtv);
    if (!SAVED) load_frame<FH, FW, kColHalo, C>(xs, p.x + static_cast<size_t>(n) * C * H * W, C, H, W, l.i0, l.j0, 4, vec);
    if (FUSED) {
        load_u_fused<C, FH, FW, 2>(us, p.g_in, p.gate_in, n, H, W, oi, oj, p.w, vec);  // u is read on frame rows [2, FH-2) only
    } else {
        load_frame<FH, FW, kColHalo, 1>(us, p.u + static_cast<size_t>(n) * H * W, 1, H, W, l.i0, l.j0, 4, vec);
    }
    // gg / gb planes start as zeros: a cell outside the image, or outside the range a stage fills, then reads as
    // "contributes nothing" and the transposed correlations below need no per-tap bounds test
    for (int idx = threadIdx.x; idx < 3 * PL / 4; idx += kBlock) reinterpret_cast<float4 *>(ggx)[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();

    // ---- stage 2: magnitude-stage gradient on 4-pixel groups (SAVED: one round, group threadIdx.x) ------------------------
    for (int gidx = threadIdx.x; gidx < GG_ROWS * GG_GX; gidx += kBlock) {
        const Group q = group_of<GG_GX, 2, 2>(gidx, oi, oj, H, W);
        if (q.in) {
            float b[SAVED ? 1 : C][3][6];
            if constexpr (!SAVED) blur_group<C, FH, FW>(xs, wt, q.fr - 2, q.fc - 2, q.i, q.jb, H, W, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = q.jb + k, o = q.fr * FW + q.fc + k;
                if (j >= 0 && j < W && q.fc + k < FW) {
                    float gx1, gy1;
                    if constexpr (SAVED) {
                        gx1 = gxv[k];
                        gy1 = gyv[k];
                    } else {
                        float ax, ay, s2, mag, mag_a, e;
                        sobel_px<C>(b, wt, k, ax, ay);
                        edge_from_sums<C>(ax, ay, p.alpha, p.high, gx1, gy1, s2, mag, mag_a, e);
                    }
                    mag_grad<C>(gx1, gy1, step125_mask(us[o], gx1, gy1, p.alpha, p.high), ggx[o], ggy[o]);
                }
            }
        }
    }
    __syncthreads();

    // ---- stages 3 + 4: gb = pad^T(Sx^T ggx + Sy^T ggy), barrier, out = pad^T(G^T gb) on this lane's 4 pixels ------------
    float o4[4];
    adjoint_tail<TH, TW, FW>(ggx, ggy, gb, wt, H, W, l.i0, l.j0, oi, oj, l.live, l.ti, l.tjb, o4);
    if (!l.live) return;
    by_vec(vec, [&](auto v) {
        constexpr bool VEC = decltype(v)::value;
        store_px4<VEC>(p.g_img, plane_at(n, 1, 0, H, W, l.ti, l.tjb), l.tjb, W, o4);
        if (FUSED) store_gated<C, VEC>(p.g_hfs, n, H, W, l.ti, l.tjb, gin, gtv);
    });
}

// ---- host side --------------------------------------------------------------------------------------
// forward: 16x64 / 32x32 tiles = exactly 256 four-pixel groups.  backward: 11x64 / 24x32, because its heaviest
// stage works on the (TH+4) x (TW+4) halo region: 15 x 17 = 255 (resp. 28 x 9 = 252) groups = one round of 256 lanes.
constexpr int kFwdTH64 = 16, kFwdTH32 = 32, kBwdTH64 = 11, kBwdTH32 = 24;

template <bool BWD, bool SAVED>
TilePlan plan(EdgeParams &p, int B) {
    // plenty of workgroups (> 4 per CU): total work, not the critical path of one workgroup, sets the time, and the
    // 16-row tile recomputes less halo (two rounds of stage 2, but 20/16 instead of 15/11 rows per output row)
    const bool many = static_cast<int64_t>(B) * ((p.H + kFwdTH64 - 1) / kFwdTH64) * ((p.W + 63) / 64) >= 1024;
    return tile_plan(p, B, BWD ? (many && !SAVED ? kFwdTH64 : kBwdTH64) : kFwdTH64, BWD ? kBwdTH32 : kFwdTH32);
}

template <int C, bool FUSED, bool BWD, bool SAVED>
void launch_c(const EdgeParams &p, const Weights &wt, const TilePlan &l, hipStream_t s) {
    const dim3 grid(l.grid), block(kBlock);
    if constexpr (!BWD) {
        if (l.tw == 64)
            EE_LAUNCH((edge_fwd_kernel<C, kFwdTH64, 64, FUSED>), grid, block, 0, s, p, wt);
        else
            EE_LAUNCH((edge_fwd_kernel<C, kFwdTH32, 32, FUSED>), grid, block, 0, s, p, wt);
    } else if (l.tw == 64 && l.th == kBwdTH64) {
        EE_LAUNCH((edge_bwd_kernel<C, kBwdTH64, 64, FUSED, SAVED>), grid, block, 0, s, p, wt);
    } else if (l.tw == 64) {
        if constexpr (!SAVED) EE_LAUNCH((edge_bwd_kernel<C, kFwdTH64, 64, FUSED, false>), grid, block, 0, s, p, wt);  // plan() keeps SAVED off it
    } else {
        EE_LAUNCH((edge_bwd_kernel<C, kBwdTH32, 32, FUSED, SAVED>), grid, block, 0, s, p, wt);
    }
}

// what every entry point does once its pointers are in p: the checks in the ABI's order (shape, empty batch, `missing`
// pointers), the remaining fields, the profiling scope of `family` around the launch
template <bool FUSED, bool BWD, bool SAVED = false>
int launch(EdgeParams p, bool missing, int family, int B, int C, int H, int W, const float *weights27, float alpha, float high, float w,
           void *stream) {
    int rc;
    if (ends_early(rc, B, C, H, W, kBwdTH64, missing || !weights27)) return rc;
    finish_params(p, H, W, alpha, high, w);
    const Weights wt = load_weights(weights27);
    const TilePlan l = plan<BWD, SAVED>(p, B);
    hipStream_t s = as_stream(stream);
    ProfScope prof(family, s);
    switch (C) {
        case 1: launch_c<1, FUSED, BWD, SAVED>(p, wt, l, s); break;
        case 2: launch_c<2, FUSED, BWD, SAVED>(p, wt, l, s); break;
        case 3: launch_c<3, FUSED, BWD, SAVED>(p, wt, l, s); break;
        default: launch_c<4, FUSED, BWD, SAVED>(p, wt, l, s); break;
    }
    return launch_status();
}

}  // namespace

EE_API int ee_edge125_fwd_f32(const float *x, int B, int C, int H, int W, const float *weights27, float alpha, float high,
                              float *edge, float *mag, void *stream) {
    EdgeParams p{};
    p.x = x;
    p.edge = edge;
    p.mag = mag;
    return launch<false, false>(p, !x || !edge, EE_K_EDGE_FWD, B, C, H, W, weights27, alpha, high, 0.0f, stream);
}

EE_API int ee_edge125_bwd_f32(const float *x, const float *u, int B, int C, int H, int W, const float *weights27, float alpha,
                              float high, float *g_img, void *stream) {
    EdgeParams p{};
    p.x = x;
    p.u = u;
    p.g_img = g_img;
    return launch<false, true>(p, !x || !u || !g_img, EE_K_EDGE_BWD, B, C, H, W, weights27, alpha, high, 0.0f, stream);
}

EE_API int ee_frontend_fwd_f32(const float *x, const float *x_hfs, int B, int C, int H, int W, const float *weights27,
                               float alpha, float high, float w, float *x_in, uint8_t *gate, float *edge, void *stream) {
    EdgeParams p{};
    p.x = x;
    p.x_hfs = x_hfs;
    p.x_in = x_in;
    p.gate = gate;
    p.edge = edge;
    return launch<true, false>(p, !x || !x_hfs || !x_in, EE_K_FRONTEND_FWD, B, C, H, W, weights27, alpha, high, w, stream);
}

EE_API int ee_frontend_bwd_f32(const float *g_in, const uint8_t *gate, const float *x, int B, int C, int H, int W,
                               const float *weights27, float alpha, float high, float w, float *g_hfs, float *g_edge,
                               void *stream) {
    EdgeParams p{};
    p.x = x;
    p.g_in = g_in;
    p.gate_in = gate;
    p.g_hfs = g_hfs;
    p.g_img = g_edge;
    return launch<true, true>(p, !g_in || !gate || !x || !g_hfs || !g_edge, EE_K_FRONTEND_BWD, B, C, H, W, weights27, alpha, high, w, stream);
}

// ---- the pair that keeps the Sobel responses between forward and backward --------------------------------------------------
EE_API int ee_frontend_fwd_save_f32(const float *x, const float *x_hfs, int B, int C, int H, int W, const float *weights27, float alpha,
                                    float high, float w, float *x_in, uint8_t *gate, float *edge, float *gx, float *gy, void *stream) {
    EdgeParams p{};
    p.x = x;
    p.x_hfs = x_hfs;
    p.x_in = x_in;
    p.gate = gate;
    p.edge = edge;
    p.gx_out = gx;
    p.gy_out = gy;
    return launch<true, false>(p, !x || !x_hfs || !x_in || !gx || !gy, EE_K_FRONTEND_FWD, B, C, H, W, weights27, alpha, high, w, stream);
}

EE_API int ee_frontend_bwd_saved_f32(const float *g_in, const uint8_t *gate, const float *gx, const float *gy, int B, int C, int H, int W,
                                     const float *weights27, float alpha, float high, float w, float *g_hfs, float *g_edge, void *stream) {
    EdgeParams p{};
    p.g_in = g_in;
    p.gate_in = gate;
    p.gx_in = gx;
    p.gy_in = gy;
    p.g_hfs = g_hfs;
    p.g_img = g_edge;
    return launch<true, true, true>(p, !g_in || !gate || !gx || !gy || !g_hfs || !g_edge, EE_K_FRONTEND_BWD, B, C, H, W, weights27, alpha, high, w,
                                    stream);
}
