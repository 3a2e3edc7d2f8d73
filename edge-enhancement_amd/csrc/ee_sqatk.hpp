// ee_sqatk.hpp - what the three Square attacks (ee_sqatk.hip: Linf; ee_sqatk_l2.hip: L2; ee_sqatk_l1.hip: L1) share: the Philox stream
// ids, the window draw of proposal i and sample b, and the entry points' shape and pointer checks.  One definition each, so that a window
// of an L2 run is the window a Linf run would draw.
#pragma once

#include <initializer_list>

#include "ee_common.hpp"

namespace ee {

// Philox stream ids; 0 (the default), 7 (ee_net2.hip) and 15 (kStreamFabStart, ee_common.hpp) are taken
constexpr uint32_t kStreamWindow = 11u;   // window 1 of a proposal (both norms)
constexpr uint32_t kStreamStripe = 12u;   // the striped start (Linf)
constexpr uint32_t kStreamWindow2 = 13u;  // window 2 of a proposal (L2)
constexpr uint32_t kStreamTile = 14u;     // the tiles of the start (L2)

// the s x s window of proposal `it` for sample b: rows vh .. vh+s-1, columns vw .. vw+s-1, and the two words of the draw that are left
struct WindowDraw {
    int vh, vw;
    uint32_t z, w;
};

__device__ __forceinline__ WindowDraw draw_window(const Philox &ph, int it, int64_t b, int s, int H, int W, uint32_t stream_id) {
    const uint4 d = ph((static_cast<uint64_t>(static_cast<uint32_t>(it)) << 32) | static_cast<uint32_t>(b), stream_id);
    WindowDraw r;
    r.vh = static_cast<int>(__umulhi(d.x, static_cast<uint32_t>(H - s + 1)));
    r.vw = static_cast<int>(__umulhi(d.y, static_cast<uint32_t>(W - s + 1)));
    r.z = d.z;
    r.w = d.w;
    return r;
}

// B, C, H, W of an image batch whose element count and per-sample size fit the kernels' arithmetic
static inline int sqatk_check_shape(int B, int C, int H, int W) {
    if (B < 0 || C < 1 || H < 1 || W < 1) return EE_ERR_SHAPE;
    if (static_cast<int64_t>(C) * H * W > INT32_MAX) return EE_ERR_SHAPE;
    if (C > 32) return EE_ERR_UNSUPPORTED;  // one sign bit per channel in a 32-bit draw
    return EE_OK;
}

// The pointers of an init or step launch, whatever the norm: EE_ERR_NULL, then EE_ERR_ALIGN.  `need` (the images and the launch's own
// extras) must be there; `tables` (sizes, eta_off, eta of a step) only when the launch reads them, n_sizes > 0.  All are 4-byte aligned,
// the seed 8-byte.
static inline int sqatk_check_ptrs(const int64_t *seed, std::initializer_list<const void *> need, bool read_tables = false,
                                   std::initializer_list<const void *> tables = {}) {
    bool null = !seed, skew = (reinterpret_cast<uintptr_t>(seed) & 7u) != 0;
    for (const void *p : need) null |= !p, skew |= !aligned4(p);
    for (const void *p : tables) null |= read_tables && !p, skew |= !aligned4(p);
    return null ? EE_ERR_NULL : skew ? EE_ERR_ALIGN : EE_OK;
}

}  // namespace ee
