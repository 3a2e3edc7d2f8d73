// ee_bn.hip - BatchNorm2d fused with the residual add and the ReLU that follow it in every ResNet block
// (Tiny_ImageNet/models_tinyimagenet/resnet.py:44-59: out = relu(bn(conv(x)) [+ residual])).
//
// Why it exists: at the reference batch size (100 x 64x64 images) one PGD iteration of ResNet-18 is ~170 kernel
// launches averaging ~12 us, so the attack loop is launch-bound; BatchNorm -> (+ residual) -> ReLU are three (forward)
// and two (backward) launches per layer of pure HBM-bound element-wise work.  Fused: one launch each way, the
// normalised tensor is written once, and the ReLU mask is taken from the output instead of a saved copy.
//
// Seven kernel families.  The first three serve ee_bn_act_fwd/bwd_f32, which picks per shape:
//   cached   HW % 4 == 0, 16-B aligned, B * HW / 4 <= 7168 (cached_variant): one workgroup per channel - up to four on few-channel
//            layers (cached_parts) - holds the channel in registers: one read pass, all loads of a lane in flight together.
//            Every layer but the stem at the reference batch.
//   split    aligned channels too large for that, given a workspace: cut into slices (split_slices), one workgroup each; partial
//            statistics through the workspace, a second launch recombines and applies.  The 64-channel stem.
//   generic  everything else (no workspace, unaligned, HW % 4 != 0): one workgroup per channel, three passes over memory.
// The other four have entry points of their own, on the machinery of the first three:
//   dual     ee_bn_dual_*: relu(bn_a(xa) + bn_b(xb)), the end of a block with a down-sampling shortcut, cached <256, *> only.
//   sum      ee_bn_sum_act_*: the block boundary of a pre-activation network, bn(x + res); the cached kernels' SUM / ADD flags.
//   pool     ee_bn_relu_pool_*: the stem's relu(bn(x)) -> MaxPool2d(3, 2, 1) without the full-resolution activation.
//   sync     ee_syncbn_*: SyncBatchNorm's local halves around the two collectives, on the split kernels.
// Training mode: mean, then centred variance (two-pass, fp32, fixed-order wave / workgroup reductions -> bit-reproducible), then
// normalise + add + ReLU.  Running statistics are updated in the kernel exactly as nn.BatchNorm2d does (momentum, unbiased
// variance).  NCHW fp32.  Every per-element and per-channel expression is one of ee_bn_math.hpp's, which is what makes the
// families (and the convolutions of ee_fuse.hpp) agree bit for bit.
//
// This is CNN-body glue, not one of SURVEY.md section 8's rows: parity is "logits within 1e-4" through the model tests.
#include "ee_bn_math.hpp"

#include <type_traits>

namespace {

using namespace ee;

template <int NT>
__device__ __forceinline__ float block_sum(float v, float *scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();  // scratch may still be read from a previous call
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += scratch[w];
    return t;
}

// two / three sums through ONE pair of barriers (round 4: the backward kernels reduced their sums one after the other, four or six
// barriers of up to sixteen wavefronts); each sum is formed exactly as block_sum forms it: the same bits.  scratch: NV * NT / 64 floats.
template <int NT, int NV>
__device__ __forceinline__ void block_sums(float (&v)[NV], float *scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += __shfl_xor(v[k], off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();  // scratch may still be read from a previous call
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) scratch[k * (NT / 64) + wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += scratch[k * (NT / 64) + w];
        v[k] = t;
    }
}

struct BnShape {
    int B, C, HW;
};

template <int NT>
__device__ __forceinline__ void block_sum_pair(float &a, float &b, float *scratch) {
    float two[2] = {a, b};
    block_sums<NT, 2>(two, scratch);
    a = two[0], b = two[1];
}

// y = [relu]((v - mean) * a + b0 [+ q])
template <bool RELU, bool RES>
__device__ __forceinline__ float4 bn_out4(float4 v, float4 q, float mean, float a, float b0) {
    float4 r = bn_affine4(v, mean, a, b0);
    if (RES) r = add4(r, q);
    return RELU ? relu_nan4(r) : r;
}

__device__ __forceinline__ void put_param_grads(float *dgamma, float *dbeta, int c, float sdz, float sdzx) {
    if (dgamma) dgamma[c] = sdzx;
    if (dbeta) dbeta[c] = sdz;
}

// element e (0 .. B*HW) of channel c lives at ((b*C + c)*HW + p), b = e / HW, p = e % HW; VEC = 4 walks float4s (HW % 4 == 0)
template <int NT, int VEC, class F>
__device__ __forceinline__ void for_channel(const BnShape s, int c, F f) {
    const int per = s.HW / VEC;
    const int total = s.B * per;
    for (int e = threadIdx.x; e < total; e += NT) {
        const int b = e / per, q = e - b * per;
        f((static_cast<size_t>(b) * s.C + c) * s.HW + static_cast<size_t>(q) * VEC);
    }
}

template <int NT, int VEC, bool RELU, bool RES>
__global__ __launch_bounds__(NT) void bn_fwd_kernel(const float *__restrict__ x, const float *__restrict__ res, const float *__restrict__ gamma,
                                                    const float *__restrict__ beta, float *running_mean, float *running_var, float momentum,
                                                    float eps, int training, float *__restrict__ y, float *__restrict__ save_mean,
                                                    float *__restrict__ save_invstd, BnShape s) {
    __shared__ float scratch[3 * (NT / 64)];
    const int c = blockIdx.x;
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    float mean, invstd;
    if (training) {
        float acc = 0.0f;
        for_channel<NT, VEC>(s, c, [&](size_t o) {
            if (VEC == 4) acc += quad_sum(*reinterpret_cast<const float4 *>(x + o));
            else acc += x[o];
        });
        mean = block_sum<NT>(acc, scratch) / n;
        float var = 0.0f;
        for_channel<NT, VEC>(s, c, [&](size_t o) {
            if (VEC == 4) {
                var += quad_sqdev(*reinterpret_cast<const float4 *>(x + o), mean);
            } else {
                const float a = x[o] - mean;
                var += a * a;
            }
        });
        var = block_sum<NT>(var, scratch) / n;
        invstd = bn_invstd(var, eps);
        if (threadIdx.x == 0) bn_commit_stats(c, mean, var, invstd, n, momentum, save_mean, save_invstd, running_mean, running_var);
    } else {
        const BnStats st = bn_known_stats(0, save_mean, save_invstd, running_mean, running_var, eps, c);
        mean = st.mean, invstd = st.invstd;
    }
    const float a = bn_gain(invstd, gamma, c), b0 = bn_shift(beta, c);
    for_channel<NT, VEC>(s, c, [&](size_t o) {
        if (VEC == 4) {
            const float4 q = RES ? *reinterpret_cast<const float4 *>(res + o) : zero4();
            *reinterpret_cast<float4 *>(y + o) = bn_out4<RELU, RES>(*reinterpret_cast<const float4 *>(x + o), q, mean, a, b0);
        } else {
            float r = bn_affine(x[o], mean, a, b0);
            if (RES) r += res[o];
            if (RELU) r = relu_nan(r);
            y[o] = r;
        }
    });
}

// backward.  dz = RELU ? dy * (y > 0) : dy  (threshold_backward); dres = dz (the residual branch's gradient);
// training: dx = gamma*invstd * (dz - mean(dz) - xhat * mean(dz*xhat));  eval: dx = gamma*invstd_running * dz.
// The gradient may arrive in two pieces (the block output feeds the next block's convolution AND its identity branch; autograd
// would add them in a separate launch): dy + dy2, the same fp32 add, on load.
template <int NT, int VEC, bool RELU>
__global__ __launch_bounds__(NT) void bn_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                    const float *__restrict__ x, const float *__restrict__ beta,
                                                    const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                    const float *__restrict__ save_invstd, const float *__restrict__ running_mean,
                                                    const float *__restrict__ running_var, float eps, int training, float *__restrict__ dx,
                                                    float *__restrict__ dres, float *__restrict__ dgamma, float *__restrict__ dbeta, BnShape s) {
    __shared__ float scratch[3 * (NT / 64)];
    const int c = blockIdx.x;
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    const BnStats st = bn_known_stats(training, save_mean, save_invstd, running_mean, running_var, eps, c);
    const float mean = st.mean, invstd = st.invstd;
    const MaskArgs mk = mask_args(y, gamma, beta, invstd, c);
    auto masked4 = [&](size_t o, float4 v) {
        float4 g = *reinterpret_cast<const float4 *>(dy + o);
        if (dy2) g = add4(g, *reinterpret_cast<const float4 *>(dy2 + o));
        if (RELU) g = mask4(g, mk.on ? bn_affine4(v, mean, mk.a, mk.b0) : *reinterpret_cast<const float4 *>(y + o));
        return g;
    };
    auto masked1 = [&](size_t o, float v) {
        float g = dy2 ? dy[o] + dy2[o] : dy[o];
        if (RELU) g = mask1(g, mk.on ? bn_affine(v, mean, mk.a, mk.b0) : y[o]);
        return g;
    };
    float sdz = 0.0f, sdzx = 0.0f;
    for_channel<NT, VEC>(s, c, [&](size_t o) {
        if (VEC == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(x + o);
            const float4 g = masked4(o, v);
            sdz += quad_sum(g);
            sdzx += quad_dot(g, bn_xhat4(v, mean, invstd));
        } else {
            const float v = x[o];
            const float g = masked1(o, v);
            sdz += g;
            sdzx += g * bn_xhat(v, mean, invstd);
        }
    });
    block_sum_pair<NT>(sdz, sdzx, scratch);
    if (threadIdx.x == 0) put_param_grads(dgamma, dbeta, c, sdz, sdzx);
    const float w = bn_gain(invstd, gamma, c);
    const float m1 = training ? sdz / n : 0.0f, m2 = training ? sdzx / n : 0.0f;
    for_channel<NT, VEC>(s, c, [&](size_t o) {
        if (VEC == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(x + o);
            const float4 g = masked4(o, v);
            if (dres) *reinterpret_cast<float4 *>(dres + o) = g;
            if (dx) *reinterpret_cast<float4 *>(dx + o) = bn_dx4(w, g, m1, bn_xhat4(v, mean, invstd), m2);
        } else {
            const float v = x[o];
            const float g = masked1(o, v);
            if (dres) dres[o] = g;
            if (dx) dx[o] = bn_dx(w, g, m1, bn_xhat(v, mean, invstd), m2);
        }
    });
}

// ---- register-cached variants: a channel that fits MAXV float4s per lane is read from memory ONCE (the two-pass
// statistics and the normalisation run on registers), which removes two of the three dependent L2 round trips -------------

// float4 offsets of a lane's MAXV register slots in channel c; load(j) then reads slot j.  A slot past the channel's end gets the
// offset of the channel's last element, so every slot is loaded unconditionally - MAXV loads in flight - and masked afterwards
// (slot_valid): a load under a predicate becomes a branch with its own s_waitcnt, i.e. MAXV serialised memory round trips.
template <int NT, int MAXV, class L>
__device__ __forceinline__ void load_channel(const BnShape s, int c, unsigned (&off)[MAXV], L load) {
    const int per = s.HW / 4, total = s.B * per;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int e0 = threadIdx.x + j * NT;
        const int e = e0 < total ? e0 : total - 1;
        const int b = e / per, q = e - b * per;
        off[j] = static_cast<unsigned>(b * s.C + c) * static_cast<unsigned>(per) + static_cast<unsigned>(q);
        load(j);
    }
}
template <int NT>
__device__ __forceinline__ bool slot_valid(int j, int total) {
    return static_cast<int>(threadIdx.x) + j * NT < total;
}

// gridDim.y = P workgroups per channel (few-channel layers: 64 channels fill 64 of 256 CUs).  Every one of them reads the whole
// channel and forms the SAME sums in the same order (the same bits); part p then finishes and stores only the register slots it owns -
// a quarter of the stores per CU - and part 0 owns the per-channel side effects.
template <int MAXV>
__device__ __forceinline__ bool owns_slot(int j, int P, int part) {
    return j * P / MAXV == part;
}
// a tensor that only the last pass needs (the forward's residual, the backward's dadd), so only for the slots the part owns; the slots
// of other parts load this part's first own slot again - unconditional, and no traffic
template <int MAXV>
__device__ __forceinline__ void load_own_slots(const float4 *p, const unsigned (&off)[MAXV], int P, int part, float4 (&v)[MAXV]) {
    const int jf = (part * MAXV + P - 1) / P;  // (smallest j with j * P / MAXV == part)
    unsigned of = off[0];
#pragma unroll
    for (int j = 1; j < MAXV; ++j) of = j == jf ? off[j] : of;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) v[j] = p[owns_slot<MAXV>(j, P, part) ? off[j] : of];
}

struct BnParams {
    const float *gamma, *beta;
    float *running_mean, *running_var;
    float momentum, eps;
    float *save_mean, *save_invstd;
};

// mean and invstd of the channel held in xv (lanes past the end hold zeros); in training mode the workgroup with `writer` commits them
template <int NT, int MAXV>
__device__ __forceinline__ void cached_stats(const float4 (&xv)[MAXV], int total, float n, const BnParams &p, int training, int c, float *scratch,
                                             bool writer, float &mean, float &invstd) {
    if (training) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXV; ++j) acc += quad_sum(xv[j]);
        mean = block_sum<NT>(acc, scratch) / n;
        float var = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXV; ++j)
            if (slot_valid<NT>(j, total)) var += quad_sqdev(xv[j], mean);
        var = block_sum<NT>(var, scratch) / n;
        invstd = bn_invstd(var, p.eps);
        if (threadIdx.x == 0 && writer) bn_commit_stats(c, mean, var, invstd, n, p.momentum, p.save_mean, p.save_invstd, p.running_mean, p.running_var);
    } else {
        const BnStats st = bn_known_stats(0, p.save_mean, p.save_invstd, p.running_mean, p.running_var, p.eps, c);
        mean = st.mean, invstd = st.invstd;
    }
}

// SUM (ee_bn_sum_act_fwd_f32, the block boundary of a pre-activation network): the statistics and the normalisation are those of
// s = x + res, so every part reads the residual for ALL its register slots; s goes to sum_out (nullable) for the part's own slots.
// RES and SUM are never both set.
template <int NT, int MAXV, bool RELU, bool RES, bool SUM = false>
__global__ __launch_bounds__(NT) void bn_fwd_cached_kernel(const float *__restrict__ x, const float *__restrict__ res,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           float *running_mean, float *running_var, float momentum, float eps, int training,
                                                           float *__restrict__ y, float *__restrict__ save_mean,
                                                           float *__restrict__ save_invstd, BnShape s, float *__restrict__ sum_out) {
    __shared__ float scratch[3 * (NT / 64)];
    const int c = blockIdx.x;
    const int P = static_cast<int>(gridDim.y), part = static_cast<int>(blockIdx.y);
    const int total = s.B * (s.HW / 4);
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    const float4 *x4 = reinterpret_cast<const float4 *>(x), *r4 = reinterpret_cast<const float4 *>(res);
    float4 xv[MAXV], rv[(RES || SUM) ? MAXV : 1];
    unsigned off[MAXV];
    load_channel<NT, MAXV>(s, c, off, [&](int j) { xv[j] = x4[off[j]]; });
    if constexpr (SUM) {
#pragma unroll
        for (int j = 0; j < MAXV; ++j) rv[j] = r4[off[j]];
#pragma unroll
        for (int j = 0; j < MAXV; ++j) xv[j] = add4(xv[j], rv[j]);  // one fp32 add per element, as the reference's `out += shortcut`
    }
    if constexpr (RES) load_own_slots(r4, off, P, part, rv);  // its latency hides behind the statistics
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (!slot_valid<NT>(j, total)) xv[j] = zero4();
    float mean, invstd;
    cached_stats<NT, MAXV>(xv, total, n, BnParams{gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd}, training, c, scratch,
                           part == 0, mean, invstd);
    const float a = bn_gain(invstd, gamma, c), b0 = bn_shift(beta, c);
    float4 *y4 = reinterpret_cast<float4 *>(y);
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (slot_valid<NT>(j, total) && owns_slot<MAXV>(j, P, part)) {
            if (SUM && sum_out) reinterpret_cast<float4 *>(sum_out)[off[j]] = xv[j];
            y4[off[j]] = bn_out4<RELU, RES>(xv[j], rv[RES ? j : 0], mean, a, b0);
        }
}

// ADD (ee_bn_sum_act_bwd_f32): dx += dadd on store - the gradient that reaches the normalised sum through the next block's identity branch
template <int NT, int MAXV, bool RELU, bool ADD = false>
__global__ __launch_bounds__(NT) void bn_bwd_cached_kernel(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                           const float *__restrict__ x, const float *__restrict__ beta,
                                                           const float *__restrict__ gamma, const float *__restrict__ save_mean,
                                                           const float *__restrict__ save_invstd, const float *__restrict__ running_mean,
                                                           const float *__restrict__ running_var, float eps, int training,
                                                           float *__restrict__ dx, float *__restrict__ dres, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta, BnShape s, const float *__restrict__ dadd) {
    __shared__ float scratch[3 * (NT / 64)];
    const int c = blockIdx.x;
    const int P = static_cast<int>(gridDim.y), part = static_cast<int>(blockIdx.y);
    const int total = s.B * (s.HW / 4);
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    const BnStats st = bn_known_stats(training, save_mean, save_invstd, running_mean, running_var, eps, c);
    const float mean = st.mean, invstd = st.invstd;
    const float4 *dy4 = reinterpret_cast<const float4 *>(dy), *y4 = reinterpret_cast<const float4 *>(y), *x4 = reinterpret_cast<const float4 *>(x);
    const float4 *dy24 = reinterpret_cast<const float4 *>(dy2);
    float4 gv[MAXV], hv[MAXV], yv[RELU ? MAXV : 1], av[ADD ? MAXV : 1];  // masked gradient dz, xhat, y, dadd
    unsigned off[MAXV];
    load_channel<NT, MAXV>(s, c, off, [&](int j) {
        gv[j] = dy4[off[j]];
        hv[j] = x4[off[j]];
        if (RELU && y4) yv[j] = y4[off[j]];
    });
    if constexpr (ADD) load_own_slots(reinterpret_cast<const float4 *>(dadd), off, P, part, av);
    const MaskArgs mk = mask_args(y, gamma, beta, invstd, c);
    if (dy24) {
#pragma unroll
        for (int j = 0; j < MAXV; ++j) gv[j] = add4(gv[j], dy24[off[j]]);
    }
    float sdz = 0.0f, sdzx = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        float4 g = gv[j];
        const float4 v = hv[j];
        if (RELU) g = mask4(g, mk.on ? bn_affine4(v, mean, mk.a, mk.b0) : yv[j]);
        float4 h = bn_xhat4(v, mean, invstd);
        if (!slot_valid<NT>(j, total)) g = h = zero4();
        sdz += quad_sum(g);
        sdzx += quad_dot(g, h);
        gv[j] = g;
        hv[j] = h;
    }
    block_sum_pair<NT>(sdz, sdzx, scratch);
    if (threadIdx.x == 0 && part == 0) put_param_grads(dgamma, dbeta, c, sdz, sdzx);
    const float w = bn_gain(invstd, gamma, c);
    const float m1 = training ? sdz / n : 0.0f, m2 = training ? sdzx / n : 0.0f;
    float4 *dx4 = reinterpret_cast<float4 *>(dx), *dr4 = reinterpret_cast<float4 *>(dres);
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (slot_valid<NT>(j, total) && owns_slot<MAXV>(j, P, part)) {
            if (dres) dr4[off[j]] = gv[j];
            if (dx) {
                float4 d = bn_dx4(w, gv[j], m1, hv[j], m2);
                if (ADD) d = add4(d, av[j]);
                dx4[off[j]] = d;
            }
        }
}

// ---- a residual block with a down-sampling shortcut ends in TWO BatchNorms: relu(bn2(conv2 out) + bn_ds(conv1x1 out)) (resnet.py:54-59,
// :137-142).  Both are per-channel, so one workgroup does both for its channel - one launch each way instead of two (at these sizes
// a BatchNorm launch is 5-6 us of launch floor).  Same statistics, same expressions, same order as bn_fwd/bwd_cached_kernel run one
// after the other: bit-identical results. ---------------------------------------------------------------------------------------------

// y = relu( bn_a(xa) + bn_b(xb) ): bn_b first (it is the `residual` of the unfused call), then bn_a with the residual added
template <int NT, int MAXV>
__global__ __launch_bounds__(NT) void bn_dual_fwd_cached_kernel(const float *__restrict__ xa, const float *__restrict__ xb, BnParams pa, BnParams pb,
                                                                int training, float *__restrict__ y, BnShape s) {
    __shared__ float scratch[3 * (NT / 64)];
    const int c = blockIdx.x;
    const int total = s.B * (s.HW / 4);
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    const float4 *a4 = reinterpret_cast<const float4 *>(xa), *b4 = reinterpret_cast<const float4 *>(xb);
    float4 av[MAXV], bv[MAXV];
    unsigned off[MAXV];
    load_channel<NT, MAXV>(s, c, off, [&](int j) { av[j] = a4[off[j]], bv[j] = b4[off[j]]; });
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (!slot_valid<NT>(j, total)) av[j] = bv[j] = zero4();
    float mean_b, inv_b, mean_a, inv_a;
    cached_stats<NT, MAXV>(bv, total, n, pb, training, c, scratch, true, mean_b, inv_b);
    cached_stats<NT, MAXV>(av, total, n, pa, training, c, scratch, true, mean_a, inv_a);
    const float sb = bn_gain(inv_b, pb.gamma, c), tb = bn_shift(pb.beta, c);
    const float sa = bn_gain(inv_a, pa.gamma, c), ta = bn_shift(pa.beta, c);
    float4 *y4 = reinterpret_cast<float4 *>(y);
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (slot_valid<NT>(j, total)) y4[off[j]] = bn_out4<true, true>(av[j], bn_affine4(bv[j], mean_b, sb, tb), mean_a, sa, ta);
}

// dz = (y > 0) * (dy + dy2); bn_a's backward on dz -> dxa, then bn_b's (no ReLU of its own) on the same dz -> dxb
template <int NT, int MAXV>
__global__ __launch_bounds__(NT) void bn_dual_bwd_cached_kernel(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                                const float *__restrict__ xa, const float *__restrict__ xb, BnParams pa, BnParams pb,
                                                                int training, float *__restrict__ dxa, float *__restrict__ dxb,
                                                                float *__restrict__ dgamma_a, float *__restrict__ dbeta_a,
                                                                float *__restrict__ dgamma_b, float *__restrict__ dbeta_b, BnShape s) {
    __shared__ float scratch[3 * (NT / 64)];
    const int c = blockIdx.x;
    const int total = s.B * (s.HW / 4);
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    const BnStats a = bn_known_stats(training, pa.save_mean, pa.save_invstd, pa.running_mean, pa.running_var, pa.eps, c);
    const BnStats b = bn_known_stats(training, pb.save_mean, pb.save_invstd, pb.running_mean, pb.running_var, pb.eps, c);
    const float4 *dy4 = reinterpret_cast<const float4 *>(dy), *dy24 = reinterpret_cast<const float4 *>(dy2), *y4 = reinterpret_cast<const float4 *>(y);
    const float4 *a4 = reinterpret_cast<const float4 *>(xa), *b4 = reinterpret_cast<const float4 *>(xb);
    float4 gv[MAXV], ha[MAXV], hb[MAXV], yv[MAXV];
    unsigned off[MAXV];
    load_channel<NT, MAXV>(s, c, off, [&](int j) {
        gv[j] = dy4[off[j]];
        ha[j] = a4[off[j]];
        hb[j] = b4[off[j]];
        yv[j] = y4[off[j]];
    });
    if (dy24) {
#pragma unroll
        for (int j = 0; j < MAXV; ++j) gv[j] = add4(gv[j], dy24[off[j]]);
    }
    float sdz = 0.0f, sa = 0.0f, sb = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        float4 g = mask4(gv[j], yv[j]);
        float4 xa_ = bn_xhat4(ha[j], a.mean, a.invstd), xb_ = bn_xhat4(hb[j], b.mean, b.invstd);
        if (!slot_valid<NT>(j, total)) g = xa_ = xb_ = zero4();
        sdz += quad_sum(g);
        sa += quad_dot(g, xa_);
        sb += quad_dot(g, xb_);
        gv[j] = g;
        ha[j] = xa_;
        hb[j] = xb_;
    }
    {
        float three[3] = {sdz, sa, sb};
        block_sums<NT, 3>(three, scratch);
        sdz = three[0], sa = three[1], sb = three[2];
    }
    if (threadIdx.x == 0) {
        put_param_grads(dgamma_a, dbeta_a, c, sdz, sa);
        put_param_grads(dgamma_b, dbeta_b, c, sdz, sb);
    }
    const float wa = bn_gain(a.invstd, pa.gamma, c), wb = bn_gain(b.invstd, pb.gamma, c);
    const float m1 = training ? sdz / n : 0.0f, ma = training ? sa / n : 0.0f, mb = training ? sb / n : 0.0f;
    float4 *da4 = reinterpret_cast<float4 *>(dxa), *db4 = reinterpret_cast<float4 *>(dxb);
#pragma unroll
    for (int j = 0; j < MAXV; ++j)
        if (slot_valid<NT>(j, total)) {
            if (dxa) da4[off[j]] = bn_dx4(wa, gv[j], m1, ha[j], ma);
            if (dxb) db4[off[j]] = bn_dx4(wb, gv[j], m1, hb[j], mb);
        }
}

// workgroups per channel of the register-cached kernels: as many as keep the grid within the chip (layer1's 64 channels: 4; 128: 2), at most one
// per register slot
inline int cached_parts(int C, int maxv) {
    static const int off = [] { const char *e = getenv("EEADV_BN_PARTS"); return (e && e[0] == '0') ? 1 : 0; }();
    if (off) return 1;
    int p = device_cus() / (C > 0 ? C : 1);
    p = p > 4 ? 4 : p;
    p = p > maxv ? maxv : p;
    return p < 1 ? 1 : p;
}

// which cached variant holds a channel of `quads` float4s: 0 = none
inline int cached_variant(int64_t quads, int64_t numel) {
    if (numel / 4 > 0xffffffffLL) return 0;  // 32-bit float4 offsets
    if (quads <= 2 * 256) return 1;          // <256, 2>
    if (quads <= 7 * 256) return 2;          // <256, 7>
    if (quads <= 7 * 1024) return 3;         // <1024, 7>
    return 0;
}

// ---- host side: from run-time flags to template arguments ------------------------------------------------------------------------------
// dispatch(flag, f) calls f(std::true_type{}) or f(std::false_type{}); with two flags, f(A, B)
template <class F>
void dispatch(bool a, F f) {
    if (a) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
void dispatch(bool a, bool b, F f) {
    dispatch(a, [&](auto A) { dispatch(b, [&](auto B) { f(A, B); }); });
}

// cached_variant's number as the cached kernels' <NT, MAXV>: f(CachedCfg<NT, MAXV>{}); false: cv names no cached variant
template <int NT_, int MAXV_>
struct CachedCfg {
    static constexpr int NT = NT_, MAXV = MAXV_;
};
template <class F>
bool with_cached_cfg(int cv, F f) {
    if (cv == 1) f(CachedCfg<256, 2>{});
    else if (cv == 2) f(CachedCfg<256, 7>{});
    else if (cv == 3) f(CachedCfg<1024, 7>{});
    else return false;
    return true;
}

// the arguments that the generic, cached and split kernels of a direction share, in the kernels' order; `tail`: what follows them
struct FwdArgs {
    const float *x, *res, *gamma, *beta;
    float *running_mean, *running_var;
    float momentum, eps;
    int training;
    float *y, *save_mean, *save_invstd;
};
struct BwdArgs {
    const float *dy, *dy2, *y, *x, *beta, *gamma, *save_mean, *save_invstd, *running_mean, *running_var;
    float eps;
    int training;
    float *dx, *dres, *dgamma, *dbeta;
};
template <class K, class... Tail>
void launch_fwd_args(K kernel, dim3 grid, dim3 block, hipStream_t st, const FwdArgs &a, Tail... tail) {
    EE_LAUNCH(kernel, grid, block, 0, st, a.x, a.res, a.gamma, a.beta, a.running_mean, a.running_var, a.momentum, a.eps, a.training, a.y, a.save_mean,
              a.save_invstd, tail...);
}
template <class K, class... Tail>
void launch_bwd_args(K kernel, dim3 grid, dim3 block, hipStream_t st, const BwdArgs &a, Tail... tail) {
    EE_LAUNCH(kernel, grid, block, 0, st, a.dy, a.dy2, a.y, a.x, a.beta, a.gamma, a.save_mean, a.save_invstd, a.running_mean, a.running_var, a.eps,
              a.training, a.dx, a.dres, a.dgamma, a.dbeta, tail...);
}

// sum_out: the SUM form (ee_bn_sum_act_fwd_f32: a.res is added BEFORE the statistics; never together with RES); `sum` says so, as
// sum_out itself may be null
template <int NT, int MAXV>
void launch_fwd_cached(bool relu, bool sum, hipStream_t st, const FwdArgs &a, BnShape s, float *sum_out) {
    const dim3 grid(static_cast<unsigned>(s.C), static_cast<unsigned>(cached_parts(s.C, MAXV))), block(NT);
    if (sum)
        dispatch(relu, [&](auto R) { launch_fwd_args(bn_fwd_cached_kernel<NT, MAXV, decltype(R)::value, false, true>, grid, block, st, a, s, sum_out); });
    else
        dispatch(relu, a.res != nullptr, [&](auto R, auto Q) {
            launch_fwd_args(bn_fwd_cached_kernel<NT, MAXV, decltype(R)::value, decltype(Q)::value>, grid, block, st, a, s, sum_out);
        });
}

// dadd: ee_bn_sum_act_bwd_f32's gradient from the identity branch, or null
template <int NT, int MAXV>
void launch_bwd_cached(bool relu, hipStream_t st, const BwdArgs &a, BnShape s, const float *dadd) {
    const dim3 grid(static_cast<unsigned>(s.C), static_cast<unsigned>(cached_parts(s.C, MAXV))), block(NT);
    dispatch(relu, dadd != nullptr, [&](auto R, auto A) {
        launch_bwd_args(bn_bwd_cached_kernel<NT, MAXV, decltype(R)::value, decltype(A)::value>, grid, block, st, a, s, dadd);
    });
}


// ---- split variants: a channel too large for one workgroup's registers (the ResNet stem: 102 400 values per channel at the
// reference batch, only 64 channels) is cut into S slices, one workgroup each, in two launches: partial statistics into a
// small workspace, then every workgroup recombines the S partials in the same fixed order (Chan's parallel variance
// update, so the two-pass accuracy is kept) and handles its slice.  One workgroup per channel left 3/4 of the chip idle
// and ran at the per-CU L2 bandwidth (35 us forward / 50 us backward for the stem, rocprofv3). --------------------------
constexpr int SPLIT_NT = 256;
constexpr int SPLIT_MAX = 64;

inline int split_slices(int64_t quads) {
    const int64_t s = (quads + 2047) / 2048;
    return static_cast<int>(s < 1 ? 1 : (s > SPLIT_MAX ? SPLIT_MAX : s));
}

struct Slice {
    int begin, end;  // float4 index range inside the channel
};
__device__ __forceinline__ Slice my_slice(int total, int S, int s) {
    const int chunk = (total + S - 1) / S;
    const int b = s * chunk, e = b + chunk;
    return {b < total ? b : total, e < total ? e : total};
}

// walks the slice four elements per lane at a time: `load` (memory only, no side effects) runs unconditionally on clamped
// offsets for all four - four round trips in flight - and `use` then runs on the valid ones
template <class L, class U>
__device__ __forceinline__ void for_slice(const BnShape s, int c, Slice sl, L load, U use) {
    const int per = s.HW / 4;
    if (sl.end <= sl.begin) return;
    for (int e0 = sl.begin + threadIdx.x; e0 < sl.end; e0 += 4 * SPLIT_NT) {
        size_t off[4];
        decltype(load(size_t{})) val[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e1 = e0 + u * SPLIT_NT;
            const int e = e1 < sl.end ? e1 : sl.end - 1;
            const int b = e / per, q = e - b * per;
            off[u] = (static_cast<size_t>(b) * s.C + c) * per + q;
            val[u] = load(off[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u * SPLIT_NT < sl.end) use(val[u], off[u]);
    }
}

// Chan's recombination of the S per-slice partials p[2 i + {0, 1}] = (sum, M2 about the slice's own mean) of bn_split_stats_kernel, in
// slice order: the channel's mean and M2.  The one routine behind every workgroup's statistics and SyncBatchNorm's per-rank moments.
__device__ __forceinline__ void combine_moments(const float *p, int S, int total, float n, float &mean, float &m2) {
    float sum = 0.0f;
#pragma unroll 4
    for (int i = 0; i < S; ++i) sum += p[2 * i];
    mean = sum / n;
    m2 = 0.0f;
#pragma unroll 4
    for (int i = 0; i < S; ++i) {
        const Slice sl = my_slice(total, S, i);
        const float cnt = 4.0f * static_cast<float>(sl.end - sl.begin);
        if (cnt > 0.0f) {
            const float d = p[2 * i] / cnt - mean;
            m2 += p[2 * i + 1] + cnt * (d * d);
        }
    }
}

// channel c's S pairs of a [C][S][2] workspace through LDS in ONE parallel load: a loop of dependent global loads (S up to 64) cost
// 10 us per workgroup
__device__ __forceinline__ void stage_partials(const float *__restrict__ ws, int c, int S, float *sh) {
    for (int i = threadIdx.x; i < 2 * S; i += SPLIT_NT) sh[i] = ws[static_cast<size_t>(c) * S * 2 + i];
    __syncthreads();
}
// every lane recombines the S partials itself, in slice order: identical in all workgroups
__device__ __forceinline__ void combine_slices(const float *__restrict__ ws, int c, int S, int total, float n, float *sh, float &mean, float &var) {
    stage_partials(ws, c, S, sh);
    float m2;
    combine_moments(sh, S, total, n, mean, m2);
    var = m2 / n;
}
// the backward's partials (sum dz, sum dz * xhat), summed by every lane in index order
__device__ __forceinline__ void sum_partials(const float *__restrict__ ws, int c, int S, float *sh, float &sdz, float &sdzx) {
    stage_partials(ws, c, S, sh);
    sdz = 0.0f, sdzx = 0.0f;
#pragma unroll 4
    for (int i = 0; i < S; ++i) {
        sdz += sh[2 * i];
        sdzx += sh[2 * i + 1];
    }
}

// ws[(c*S + s)*2 + {0,1}] = (sum, M2 about the slice's own mean)
__global__ __launch_bounds__(SPLIT_NT) void bn_split_stats_kernel(const float *__restrict__ x, float *__restrict__ ws, BnShape s, int S) {
    __shared__ float scratch[3 * (SPLIT_NT / 64)];
    const int c = blockIdx.x, sl_i = blockIdx.y;
    const Slice sl = my_slice(s.B * (s.HW / 4), S, sl_i);
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    float acc = 0.0f;
    for_slice(s, c, sl, [&](size_t o) { return x4[o]; }, [&](float4 v, size_t) { acc += quad_sum(v); });
    const float sum = block_sum<SPLIT_NT>(acc, scratch);
    const float cnt = 4.0f * static_cast<float>(sl.end - sl.begin);
    const float mean = cnt > 0.0f ? sum / cnt : 0.0f;
    float m2 = 0.0f;
    for_slice(s, c, sl, [&](size_t o) { return x4[o]; }, [&](float4 v, size_t) { m2 += quad_sqdev(v, mean); });
    m2 = block_sum<SPLIT_NT>(m2, scratch);
    if (threadIdx.x == 0) {
        ws[(static_cast<size_t>(c) * S + sl_i) * 2 + 0] = sum;
        ws[(static_cast<size_t>(c) * S + sl_i) * 2 + 1] = m2;
    }
}

// the forward over one slice, once the channel's statistics are known (bn_split_apply_kernel, bn_sync_apply_kernel)
template <bool RELU, bool RES>
__device__ __forceinline__ void slice_fwd_apply(const float *__restrict__ x, const float *__restrict__ res, float *__restrict__ y, BnShape s, int c,
                                                Slice sl, float mean, float a, float b0) {
    const float4 *x4 = reinterpret_cast<const float4 *>(x), *r4 = reinterpret_cast<const float4 *>(res);
    float4 *y4 = reinterpret_cast<float4 *>(y);
    struct XR {
        float4 x, r;
    };
    for_slice(s, c, sl, [&](size_t o) { return XR{x4[o], RES ? r4[o] : zero4()}; },
              [&](XR in, size_t o) { y4[o] = bn_out4<RELU, RES>(in.x, in.r, mean, a, b0); });
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(SPLIT_NT) void bn_split_apply_kernel(const float *__restrict__ x, const float *__restrict__ res,
                                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                  float *running_mean, float *running_var, float momentum, float eps,
                                                                  int training, float *__restrict__ y, float *__restrict__ save_mean,
                                                                  float *__restrict__ save_invstd, const float *__restrict__ ws, BnShape s, int S) {
    const int c = blockIdx.x, sl_i = blockIdx.y;
    const int total = s.B * (s.HW / 4);
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    float mean, invstd;
    if (training) {
        __shared__ float parts[2 * SPLIT_MAX];
        float var;
        combine_slices(ws, c, S, total, n, parts, mean, var);
        invstd = bn_invstd(var, eps);
        if (sl_i == 0 && threadIdx.x == 0) bn_commit_stats(c, mean, var, invstd, n, momentum, save_mean, save_invstd, running_mean, running_var);
    } else {
        const BnStats st = bn_known_stats(0, save_mean, save_invstd, running_mean, running_var, eps, c);
        mean = st.mean, invstd = st.invstd;
    }
    slice_fwd_apply<RELU, RES>(x, res, y, s, c, my_slice(total, S, sl_i), mean, bn_gain(invstd, gamma, c), bn_shift(beta, c));
}

struct BwdIn {
    float4 dy, y, x;
};
__device__ __forceinline__ BwdIn bwd_load(const float4 *dy4, const float4 *dy24, const float4 *y4, const float4 *x4, size_t o, bool relu, bool want_x,
                                          float mean, const MaskArgs &mk) {
    const float4 xv = (want_x || (relu && mk.on)) ? x4[o] : zero4();
    return BwdIn{dy24 ? add4(dy4[o], dy24[o]) : dy4[o], relu ? (mk.on ? bn_affine4(xv, mean, mk.a, mk.b0) : y4[o]) : zero4(), xv};
}
__device__ __forceinline__ float4 masked_dz(const BwdIn &in, bool relu) { return relu ? mask4(in.dy, in.y) : in.dy; }

// ws[(c*S + s)*2 + {0,1}] = (sum dz, sum dz*xhat) of the slice
template <bool RELU>
__global__ __launch_bounds__(SPLIT_NT) void bn_split_bwd_partial_kernel(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                                        const float *__restrict__ x, const float *__restrict__ gamma,
                                                                        const float *__restrict__ beta, const float *__restrict__ save_mean,
                                                                        const float *__restrict__ save_invstd,
                                                                        const float *__restrict__ running_mean,
                                                                        const float *__restrict__ running_var, float eps, int training,
                                                                        float *__restrict__ ws, BnShape s, int S) {
    __shared__ float scratch[3 * (SPLIT_NT / 64)];
    const int c = blockIdx.x, sl_i = blockIdx.y;
    const BnStats st = bn_known_stats(training, save_mean, save_invstd, running_mean, running_var, eps, c);
    const float mean = st.mean, invstd = st.invstd;
    const float4 *dy4 = reinterpret_cast<const float4 *>(dy), *y4 = reinterpret_cast<const float4 *>(y), *x4 = reinterpret_cast<const float4 *>(x);
    const MaskArgs mk = mask_args(y, gamma, beta, invstd, c);
    float sdz = 0.0f, sdzx = 0.0f;
    for_slice(s, c, my_slice(s.B * (s.HW / 4), S, sl_i), [&](size_t o) { return bwd_load(dy4, reinterpret_cast<const float4 *>(dy2), y4, x4, o, RELU, true, mean, mk); }, [&](BwdIn in, size_t) {
        const float4 g = masked_dz(in, RELU);
        sdz += quad_sum(g);
        sdzx += quad_dot(g, bn_xhat4(in.x, mean, invstd));
    });
    block_sum_pair<SPLIT_NT>(sdz, sdzx, scratch);
    if (threadIdx.x == 0) {
        ws[(static_cast<size_t>(c) * S + sl_i) * 2 + 0] = sdz;
        ws[(static_cast<size_t>(c) * S + sl_i) * 2 + 1] = sdzx;
    }
}

// the backward over one slice, once m1 = mean(dz) and m2 = mean(dz * xhat) are known (bn_split_bwd_apply_kernel, bn_sync_bwd_apply_kernel)
template <bool RELU>
__device__ __forceinline__ void slice_bwd_apply(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                float *__restrict__ dx, float *__restrict__ dres, BnShape s, int c, Slice sl, float mean, float invstd,
                                                float m1, float m2) {
    const float w = bn_gain(invstd, gamma, c);
    const float4 *dy4 = reinterpret_cast<const float4 *>(dy), *y4 = reinterpret_cast<const float4 *>(y), *x4 = reinterpret_cast<const float4 *>(x);
    float4 *dx4 = reinterpret_cast<float4 *>(dx), *dr4 = reinterpret_cast<float4 *>(dres);
    const bool want_x = dx != nullptr;
    const MaskArgs mk = mask_args(y, gamma, beta, invstd, c);
    for_slice(s, c, sl, [&](size_t o) { return bwd_load(dy4, reinterpret_cast<const float4 *>(dy2), y4, x4, o, RELU, want_x, mean, mk); }, [&](BwdIn in, size_t o) {
        const float4 g = masked_dz(in, RELU);
        if (dres) dr4[o] = g;
        if (dx) dx4[o] = bn_dx4(w, g, m1, bn_xhat4(in.x, mean, invstd), m2);
    });
}

template <bool RELU>
__global__ __launch_bounds__(SPLIT_NT) void bn_split_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                                      const float *__restrict__ x, const float *__restrict__ beta, const float *__restrict__ gamma,
                                                                      const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                      const float *__restrict__ running_mean,
                                                                      const float *__restrict__ running_var, float eps, int training,
                                                                      float *__restrict__ dx, float *__restrict__ dres, float *__restrict__ dgamma,
                                                                      float *__restrict__ dbeta, const float *__restrict__ ws, BnShape s, int S) {
    const int c = blockIdx.x, sl_i = blockIdx.y;
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    const BnStats st = bn_known_stats(training, save_mean, save_invstd, running_mean, running_var, eps, c);
    __shared__ float parts[2 * SPLIT_MAX];
    float sdz, sdzx;
    sum_partials(ws, c, S, parts, sdz, sdzx);
    if (sl_i == 0 && threadIdx.x == 0) put_param_grads(dgamma, dbeta, c, sdz, sdzx);
    if (!dx && !dres) return;
    slice_bwd_apply<RELU>(dy, dy2, y, x, gamma, beta, dx, dres, s, c, my_slice(s.B * (s.HW / 4), S, sl_i), st.mean, st.invstd,
                          training ? sdz / n : 0.0f, training ? sdzx / n : 0.0f);
}

// ---- the stem: relu(bn(x)) followed by MaxPool2d(3, 2, 1) (resnet.py:113-117) without the full-resolution activation -----------------
// The stem's [100,64,32,32] map is the largest tensor of the network (26 MB): writing relu(bn(x)) and reading it back for the pool,
// then - backward - writing the pool's input gradient and reading it together with y and x twice, made the stem's BatchNorm + pool
// 36 us forward and 49 us backward (242 MB of traffic).  Here the forward reads x once and writes the pooled map and its one-byte
// argmax codes (34 MB); the backward never sees a full-resolution gradient or activation: both of its passes gather the pooled
// gradient through the codes (ATen's accumulation order) and recompute the ReLU mask from x (the same expression, the same bits).
// One workgroup = one channel x a few images; a plane is staged in LDS as y = relu(bn(x)) and pooled from there with
// ee_pool.hip's scan (first maximum wins, a NaN always wins): values, codes and gradients equal the unfused sequence's bit for bit
// (the gradient sums are taken over a different partition, so dgamma / dbeta / dx agree to rounding).
struct PoolShape {
    int B, C, H, W, OH, OW, IPW, G;  // IPW images per workgroup, G = ceil(B / IPW) groups
    int nosums;                      // backward, eval mode, no parameter gradients wanted: pass 1 did not run, pass 2 needs no sums
};

// Statistics handed over by the producing convolution (ee_conv.hip: the stem forward writes, per output channel and workgroup,
// (sum, M2 about the tile's own mean, count)): one workgroup per channel merges the S partials - each lane its share in index
// order, then a fixed butterfly (Chan's update) - and writes mean / invstd and the running statistics.  3.5 us instead of the two
// passes over the 26 MB map that bn_split_stats_kernel needs.
struct Moments {
    float n, mean, m2;
};
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
    if (b.n <= 0.0f) return a;
    if (a.n <= 0.0f) return b;
    const float n = a.n + b.n, d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), (a.m2 + b.m2) + d * d * (a.n * b.n / n)};
}
__global__ __launch_bounds__(SPLIT_NT) void bn_stats_finalize_kernel(const float *__restrict__ parts, int S, float eps, float momentum,
                                                                     float *running_mean, float *running_var, float *__restrict__ save_mean,
                                                                     float *__restrict__ save_invstd) {
    __shared__ Moments sh[SPLIT_NT / 64];
    const int c = blockIdx.x;
    const float *p = parts + static_cast<size_t>(c) * S * 3;
    Moments m{0.0f, 0.0f, 0.0f};
    for (int i = threadIdx.x; i < S; i += SPLIT_NT) {
        const float n = p[3 * i + 2];
        m = merge(m, Moments{n, n > 0.0f ? p[3 * i] / n : 0.0f, p[3 * i + 1]});
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {  // lower lane first at every level: lane 0 ends with the merge in a fixed order
        Moments o{__shfl_xor(m.n, off), __shfl_xor(m.mean, off), __shfl_xor(m.m2, off)};
        m = (threadIdx.x & off) ? merge(o, m) : merge(m, o);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        Moments t = sh[0];
#pragma unroll
        for (int w = 1; w < SPLIT_NT / 64; ++w) t = merge(t, sh[w]);
        const float var = t.n > 0.0f ? t.m2 / t.n : 0.0f;
        bn_commit_stats(c, t.mean, var, bn_invstd(var, eps), t.n, momentum, save_mean, save_invstd, running_mean, running_var);
    }
}

constexpr int POOL_MERGE_MAX = 7;  // units per lane that bn_pool_fwd_kernel merges itself (1792 units: batch 112 of the 64 x 64 stem)

__global__ __launch_bounds__(SPLIT_NT) void bn_pool_fwd_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, float *running_mean, float *running_var,
                                                               float momentum, float eps, int training, float *__restrict__ yp,
                                                               uint8_t *__restrict__ code, float *__restrict__ save_mean,
                                                               float *__restrict__ save_invstd, const float *__restrict__ ws, PoolShape p, int S,
                                                               float *__restrict__ xa) {
    extern __shared__ __align__(16) float plane[];  // y = relu(bn(x)) of one image plane
    __shared__ float parts[2 * SPLIT_MAX];
    const int c = blockIdx.x, g = blockIdx.y;
    const int HW = p.H * p.W, HWq = HW / 4, OHW = p.OH * p.OW;
    const float n = static_cast<float>(p.B) * static_cast<float>(HW);
    float mean, invstd;
    if (training == 2) {  // statistics already final (bn_stats_finalize_kernel)
        mean = save_mean[c];
        invstd = save_invstd[c];
    } else if (training == 3) {
        // the producing convolution's per-unit moments (ws = [C][S][3]: sum, M2 about the unit's mean, count; S <= POOL_MERGE_MAX * SPLIT_NT) merged
        // HERE, by every workgroup of the channel the same way (the same bits): mean = sum sum_i / sum n_i, M2 = sum (M2_i + n_i (mean_i - mean)^2)
        // - two parallel sums, no chain of dependent divisions (Chan's sequential update, which made this merge 15 us in round 3) - instead of
        // a launch of its own (bn_stats_finalize_kernel: 8.5 us for 1600 units)
        const float *q = ws + static_cast<size_t>(c) * S * 3;
        float ps[POOL_MERGE_MAX], pm[POOL_MERGE_MAX], pn[POOL_MERGE_MAX];
#pragma unroll
        for (int j = 0; j < POOL_MERGE_MAX; ++j) {
            const int i = static_cast<int>(threadIdx.x) + j * SPLIT_NT, ic = i < S ? i : S - 1;
            ps[j] = q[3 * ic], pm[j] = q[3 * ic + 1], pn[j] = q[3 * ic + 2];
            if (i >= S) ps[j] = pm[j] = pn[j] = 0.0f;
        }
        float two[2] = {0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < POOL_MERGE_MAX; ++j) two[0] += ps[j], two[1] += pn[j];
        block_sums<SPLIT_NT, 2>(two, parts);
        const float cnt = two[1];
        mean = cnt > 0.0f ? two[0] / cnt : 0.0f;
        float m2 = 0.0f;
#pragma unroll
        for (int j = 0; j < POOL_MERGE_MAX; ++j) {
            const float d = (pn[j] > 0.0f ? ps[j] / pn[j] : mean) - mean;
            m2 += pm[j] + pn[j] * d * d;
        }
        __syncthreads();  // (the scratch of the first pair of sums is read)
        m2 = block_sum<SPLIT_NT>(m2, parts);
        const float var = cnt > 0.0f ? m2 / cnt : 0.0f;
        invstd = bn_invstd(var, eps);
        if (g == 0 && threadIdx.x == 0) bn_commit_stats(c, mean, var, invstd, cnt, momentum, save_mean, save_invstd, running_mean, running_var);
    } else if (training) {
        float var;
        combine_slices(ws, c, S, p.B * HWq, n, parts, mean, var);
        invstd = bn_invstd(var, eps);
        if (g == 0 && threadIdx.x == 0) bn_commit_stats(c, mean, var, invstd, n, momentum, save_mean, save_invstd, running_mean, running_var);
    } else {
        const BnStats st = bn_known_stats(0, save_mean, save_invstd, running_mean, running_var, eps, c);
        mean = st.mean, invstd = st.invstd;
    }
    const float a = bn_gain(invstd, gamma, c), b0 = bn_shift(beta, c);
    const int b_end = (g + 1) * p.IPW < p.B ? (g + 1) * p.IPW : p.B;
    for (int b = g * p.IPW; b < b_end; ++b) {
        const size_t pl = static_cast<size_t>(b) * p.C + c;
        const float4 *x4 = reinterpret_cast<const float4 *>(x) + pl * HWq;
        for (int q = threadIdx.x; q < HWq; q += SPLIT_NT) {
            reinterpret_cast<float4 *>(plane)[q] = relu_nan4(bn_affine4(x4[q], mean, a, b0));
        }
        __syncthreads();
        for (int o = threadIdx.x; o < OHW; o += SPLIT_NT) {
            const int oh = o / p.OW, ow = o - oh * p.OW;
            const int h0 = oh * 2 - 1, w0 = ow * 2 - 1;
            const int hs = h0 < 0 ? 0 : h0, wsx = w0 < 0 ? 0 : w0;
            const int he = h0 + 3 > p.H ? p.H : h0 + 3, we = w0 + 3 > p.W ? p.W : w0 + 3;
            float best = -INFINITY;
            int bc = (hs - h0) * 3 + (wsx - w0);
            for (int h = hs; h < he; ++h)
                for (int w = wsx; w < we; ++w) {
                    const float v = plane[h * p.W + w];
                    if (v > best || v != v) {  // ATen's max_pool2d: first maximum wins, a NaN always wins (ee_pool.hip)
                        best = v;
                        bc = (h - h0) * 3 + (w - w0);
                    }
                }
            yp[pl * OHW + o] = best;
            code[pl * OHW + o] = static_cast<uint8_t>(bc);
            // x at the window's argmax (optional): the backward's batch sums then need the pooled tensors only (bn_pool_bwd_sums_pooled_kernel)
            if (xa) xa[pl * OHW + o] = x[pl * HW + (h0 + bc / 3) * p.W + (w0 + bc % 3)];
        }
        __syncthreads();
    }
}

// pass 1 of the backward from POOLED tensors (round 4): a position's masked gradient dz is the sum of the pooled gradients of the windows
// whose argmax it is, so  sum dz = sum over windows (pre > 0 ? g : 0)  and  sum dz * xhat = sum over windows (pre > 0 ? g * xhat : 0)  with
// pre / xhat taken from x at the window's argmax (xa, written by the forward): 13-20 MB read instead of the 26 MB map + pooled gradient +
// codes.  Same partition and workspace as bn_pool_bwd_kernel<false>; the sums are taken in another order (rounding-level difference).
__global__ __launch_bounds__(SPLIT_NT) void bn_pool_bwd_sums_pooled_kernel(const float *__restrict__ dyp, const float *__restrict__ dyp2, const float *__restrict__ xa,
                                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                           const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                           float *__restrict__ ws, PoolShape p) {
    __shared__ float scratch[3 * (SPLIT_NT / 64)];
    const int c = blockIdx.x, g = blockIdx.y;
    const int OHW = p.OH * p.OW;
    const float mean = save_mean[c], invstd = save_invstd[c];
    const float a = bn_gain(invstd, gamma, c), b0 = bn_shift(beta, c);
    const int b_end = (g + 1) * p.IPW < p.B ? (g + 1) * p.IPW : p.B;
    float sdz = 0.0f, sdzx = 0.0f;
    for (int b = g * p.IPW; b < b_end; ++b) {
        const size_t pl = (static_cast<size_t>(b) * p.C + c) * OHW;
        for (int o0 = threadIdx.x; o0 < OHW; o0 += 4 * SPLIT_NT) {
            float gv[4], g2[4], xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // all loads first (clamped), then the arithmetic
                const int o = o0 + u * SPLIT_NT < OHW ? o0 + u * SPLIT_NT : OHW - 1;
                gv[u] = dyp[pl + o];
                g2[u] = dyp2 ? dyp2[pl + o] : 0.0f;
                xv[u] = xa[pl + o];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (o0 + u * SPLIT_NT < OHW) {
                    const float gg = dyp2 ? gv[u] + g2[u] : gv[u];
                    const float dz = mask1(gg, bn_affine(xv[u], mean, a, b0));
                    sdz += dz;
                    sdzx += dz * bn_xhat(xv[u], mean, invstd);
                }
        }
    }
    float two[2] = {sdz, sdzx};
    block_sums<SPLIT_NT, 2>(two, scratch);
    if (threadIdx.x == 0) {
        ws[(static_cast<size_t>(c) * p.G + g) * 2 + 0] = two[0];
        ws[(static_cast<size_t>(c) * p.G + g) * 2 + 1] = two[1];
    }
}

// pass 1 (APPLY = false): ws[(c*G + g)*2 + {0,1}] = (sum dz, sum dz*xhat) of the group's images; pass 2 (APPLY = true): dx
template <bool APPLY>
__global__ __launch_bounds__(SPLIT_NT) void bn_pool_bwd_kernel(const float *__restrict__ dyp, const float *__restrict__ dyp2, const uint8_t *__restrict__ code,
                                                               const float *__restrict__ x, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, const float *__restrict__ save_mean,
                                                               const float *__restrict__ save_invstd, const float *__restrict__ running_mean,
                                                               const float *__restrict__ running_var, float eps, int training,
                                                               float *__restrict__ dx, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                               float *__restrict__ ws, PoolShape p) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float scratch[3 * (SPLIT_NT / 64)];
    const int c = blockIdx.x, g = blockIdx.y;
    const int HW = p.H * p.W, HWq = HW / 4, OHW = p.OH * p.OW, Wq = p.W / 4;
    float *gp = lds;                                            // pooled gradient of one plane
    uint8_t *cd = reinterpret_cast<uint8_t *>(lds + OHW);       // its argmax codes
    const BnStats st = bn_known_stats(training, save_mean, save_invstd, running_mean, running_var, eps, c);
    const float mean = st.mean, invstd = st.invstd;
    const float a = bn_gain(invstd, gamma, c), b0 = bn_shift(beta, c);
    float m1 = 0.0f, m2 = 0.0f;
    if (APPLY && !p.nosums) {
        __shared__ float parts[2 * SPLIT_MAX];
        float sdz, sdzx;
        sum_partials(ws, c, p.G, parts, sdz, sdzx);
        if (g == 0 && threadIdx.x == 0) put_param_grads(dgamma, dbeta, c, sdz, sdzx);
        if (!dx) return;
        const float n = static_cast<float>(p.B) * static_cast<float>(HW);
        m1 = training ? sdz / n : 0.0f;
        m2 = training ? sdzx / n : 0.0f;
    }
    float sdz = 0.0f, sdzx = 0.0f;
    const int b_end = (g + 1) * p.IPW < p.B ? (g + 1) * p.IPW : p.B;
    for (int b = g * p.IPW; b < b_end; ++b) {
        const size_t pl = static_cast<size_t>(b) * p.C + c;
        for (int o = threadIdx.x; o < OHW; o += SPLIT_NT) {
            gp[o] = dyp2 ? dyp[pl * OHW + o] + dyp2[pl * OHW + o] : dyp[pl * OHW + o];
            cd[o] = code[pl * OHW + o];
        }
        __syncthreads();
        const float4 *x4 = reinterpret_cast<const float4 *>(x) + pl * HWq;
        for (int q = threadIdx.x; q < HWq; q += SPLIT_NT) {
            const float4 v4 = x4[q];
            const int h = q / Wq, w_base = 4 * (q - h * Wq);
            // the 2 x 3 candidate windows of these four pixels (ee_pool.hip: maxpool_bwd_kernel<4>), from LDS
            const int oh0 = h >> 1, ow0 = w_base >> 1;
            const bool row2 = (h & 1) && oh0 + 1 < p.OH;
            float gv[2][3];
            int cv[2][3];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const bool ok = (r == 0 || row2) && ow0 + k < p.OW;
                    const int idx = ok ? (oh0 + r) * p.OW + ow0 + k : 0;
                    gv[r][k] = ok ? gp[idx] : 0.0f;
                    cv[r][k] = ok ? cd[idx] : 255;
                }
            const float xv[4] = {v4.x, v4.y, v4.z, v4.w};
            float out[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int w = w_base + v, k0 = v >> 1;
                float acc = 0.0f;
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) {
                        if (kb == 1 && !(v & 1)) continue;  // even pixels belong to one window column only
                        const int k = k0 + kb;
                        const int want = (h - ((oh0 + r) * 2 - 1)) * 3 + (w - ((ow0 + k) * 2 - 1));
                        if (cv[r][k] == want) acc += gv[r][k];
                    }
                const float dz = mask1(acc, bn_affine(xv[v], mean, a, b0));  // the forward's expression: the same mask as y > 0
                const float xhat = bn_xhat(xv[v], mean, invstd);
                if (!APPLY) {
                    sdz += dz;
                    sdzx += dz * xhat;
                } else {
                    out[v] = bn_dx(a, dz, m1, xhat, m2);
                }
            }
            if (APPLY) reinterpret_cast<float4 *>(dx)[pl * HWq + q] = make_float4(out[0], out[1], out[2], out[3]);
        }
        __syncthreads();
    }
    if (!APPLY) {
        block_sum_pair<SPLIT_NT>(sdz, sdzx, scratch);
        if (threadIdx.x == 0) {
            ws[(static_cast<size_t>(c) * p.G + g) * 2 + 0] = sdz;
            ws[(static_cast<size_t>(c) * p.G + g) * 2 + 1] = sdzx;
        }
    }
}

inline bool pool_shape(int B, int C, int H, int W, PoolShape &p) {
    if (B < 1 || C < 1 || H < 1 || W < 4 || W % 4 || static_cast<int64_t>(H) * W > 16000) return false;  // one plane in 64 KB of LDS (ImageNet: 112 x 112)
    if (static_cast<int64_t>(B) * C * H * W / 4 > 0x7fffffffLL) return false;
    const int ipw = (B + SPLIT_MAX - 1) / SPLIT_MAX;
    p = PoolShape{B, C, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1, ipw, (B + ipw - 1) / ipw, 0};
    return true;
}

template <int NT, int VEC>
void launch_fwd(bool relu, hipStream_t st, const FwdArgs &a, BnShape s) {
    dispatch(relu, a.res != nullptr, [&](auto R, auto Q) {
        launch_fwd_args(bn_fwd_kernel<NT, VEC, decltype(R)::value, decltype(Q)::value>, dim3(static_cast<unsigned>(s.C)), dim3(NT), st, a, s);
    });
}

template <int NT, int VEC>
void launch_bwd(bool relu, hipStream_t st, const BwdArgs &a, BnShape s) {
    dispatch(relu, [&](auto R) { launch_bwd_args(bn_bwd_kernel<NT, VEC, decltype(R)::value>, dim3(static_cast<unsigned>(s.C)), dim3(NT), st, a, s); });
}


// ---- SyncBatchNorm (ImageNet/experiments_imagenet.py:125, free_imagenet/AT_free_imagenet_ddp.py:149): the batch statistics of a
// data-parallel run are those of the GLOBAL batch.  Per layer and direction the ranks exchange one small tensor (host side,
// torch.distributed over RCCL: eeadv/syncbn.py); the kernels here are the local halves around that exchange, built on the split
// kernels above (any channel size, C x S workgroups):
//   forward   bn_split_stats_kernel -> bn_moments_kernel: this rank's (mean, M2, count) per channel          -> all_gather
//             bn_sync_apply_kernel: Chan's merge of the W ranks' moments in RANK ORDER (the same bits on every rank), running
//             statistics with the global count, y = [relu]((x - mean) * invstd * gamma + beta [+ residual])
//   backward  bn_split_bwd_partial_kernel -> bn_sums_kernel: this rank's (sum dz, sum dz * xhat) per channel -> all_reduce
//             bn_sync_bwd_apply_kernel: dx = gamma * invstd * (dz - SUM dz / N - xhat * SUM dz xhat / N) with the global sums and N;
//             dgamma / dbeta stay this rank's sums (the gradient exchange of the training step averages them like every other
//             parameter gradient - torch's SyncBatchNorm does the same)
__global__ __launch_bounds__(64) void bn_moments_kernel(const float *__restrict__ ws, float *__restrict__ moments, BnShape s, int S) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= s.C) return;
    const float n = static_cast<float>(s.B) * static_cast<float>(s.HW);
    float mean, m2;
    combine_moments(ws + static_cast<size_t>(c) * S * 2, S, s.B * (s.HW / 4), n, mean, m2);
    moments[3 * c + 0] = mean;
    moments[3 * c + 1] = m2;
    moments[3 * c + 2] = n;
}

__global__ __launch_bounds__(64) void bn_sums_kernel(const float *__restrict__ ws, float *__restrict__ sums, int C, int S) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float a = 0.0f, b = 0.0f;
    for (int i = 0; i < S; ++i) {
        a += ws[(static_cast<size_t>(c) * S + i) * 2];
        b += ws[(static_cast<size_t>(c) * S + i) * 2 + 1];
    }
    sums[2 * c] = a;
    sums[2 * c + 1] = b;
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(SPLIT_NT) void bn_sync_apply_kernel(const float *__restrict__ x, const float *__restrict__ res, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, const float *__restrict__ all_moments, int W,
                                                                 float *running_mean, float *running_var, float momentum, float eps,
                                                                 float *__restrict__ y, float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                                 BnShape s, int S) {
    const int c = blockIdx.x, sl_i = blockIdx.y;
    Moments t{0.0f, 0.0f, 0.0f};
    for (int r = 0; r < W; ++r) {  // every lane of every workgroup on every rank: the same merge in the same order
        const float *m = all_moments + (static_cast<size_t>(r) * s.C + c) * 3;
        t = merge(t, Moments{m[2], m[0], m[1]});
    }
    const float var = t.n > 0.0f ? t.m2 / t.n : 0.0f;
    const float mean = t.mean, invstd = bn_invstd(var, eps);
    if (sl_i == 0 && threadIdx.x == 0) bn_commit_stats(c, mean, var, invstd, t.n, momentum, save_mean, save_invstd, running_mean, running_var);
    slice_fwd_apply<RELU, RES>(x, res, y, s, c, my_slice(s.B * (s.HW / 4), S, sl_i), mean, bn_gain(invstd, gamma, c), bn_shift(beta, c));
}

template <bool RELU>
__global__ __launch_bounds__(SPLIT_NT) void bn_sync_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ dy2, const float *__restrict__ y,
                                                                     const float *__restrict__ x, const float *__restrict__ beta, const float *__restrict__ gamma,
                                                                     const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                     const float *__restrict__ global_sums, float n_global, float *__restrict__ dx,
                                                                     float *__restrict__ dres, BnShape s, int S) {
    const int c = blockIdx.x, sl_i = blockIdx.y;
    slice_bwd_apply<RELU>(dy, dy2, y, x, gamma, beta, dx, dres, s, c, my_slice(s.B * (s.HW / 4), S, sl_i), save_mean[c], save_invstd[c],
                          global_sums[2 * c] / n_global, global_sums[2 * c + 1] / n_global);
}

inline bool al16(const void *q) { return !q || aligned16(q); }

// training mode writes the batch statistics (forward) or reads them (backward); eval mode reads the running ones
inline bool stats_ptrs_ok(int training, const float *save_mean, const float *save_invstd, const float *running_mean, const float *running_var) {
    return training ? (save_mean && save_invstd) : (running_mean && running_var);
}

// The prologue of the ee_bn_act_* / ee_bn_sum_act_* entry points.  true: return `status` now (an error, or EE_OK for an empty batch).
// tensors: the entry point's required tensor pointers are all there.
inline bool bn_args_settled(int B, int C, int HW, bool tensors, int training, const float *save_mean, const float *save_invstd, const float *running_mean,
                            const float *running_var, int &status) {
    status = EE_OK;
    if (B < 0 || C < 1 || HW < 1 || static_cast<int64_t>(B) * HW > 0x7fffffffLL) status = EE_ERR_SHAPE;
    else if (B == 0) return true;
    else if (!tensors || !stats_ptrs_ok(training, save_mean, save_invstd, running_mean, running_var)) status = EE_ERR_NULL;
    return status != EE_OK;
}

inline dim3 split_grid(int C, int S) { return dim3(static_cast<unsigned>(C), static_cast<unsigned>(S)); }

}  // namespace

// floats of workspace the split path wants for this shape; 0 = the shape runs in one workgroup per channel
EE_API int ee_bn_workspace_floats(int B, int C, int HW) {
    if (B < 1 || C < 1 || HW < 1 || HW % 4) return 0;
    const int64_t quads = static_cast<int64_t>(B) * (HW / 4);
    if (cached_variant(quads, static_cast<int64_t>(B) * C * HW) || static_cast<int64_t>(B) * C * HW / 4 > 0x7fffffffLL) return 0;
    return C * split_slices(quads) * 2;
}

EE_API int ee_bn_act_fwd_f32(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                             float *running_var, float momentum, float eps, int training, int relu, float *y, float *save_mean,
                             float *save_invstd, float *workspace, int B, int C, int HW, void *stream) {
    int status;
    if (bn_args_settled(B, C, HW, x && y, training, save_mean, save_invstd, running_mean, running_var, status)) return status;
    const BnShape s{B, C, HW};
    const FwdArgs a{x, residual, gamma, beta, running_mean, running_var, momentum, eps, training, y, save_mean, save_invstd};
    const bool vec = (HW % 4 == 0) && al16(x) && al16(y) && al16(residual);
    const bool big = static_cast<int64_t>(B) * HW >= 16384;
    const int64_t quads = static_cast<int64_t>(B) * (HW / 4), numel = static_cast<int64_t>(B) * C * HW;
    hipStream_t st = as_stream(stream);
    const bool cached = with_cached_cfg(vec ? cached_variant(quads, numel) : 0, [&](auto cfg) {
        launch_fwd_cached<decltype(cfg)::NT, decltype(cfg)::MAXV>(relu != 0, false, st, a, s, nullptr);
    });
    if (cached) {
    } else if (vec && workspace && numel / 4 <= 0x7fffffffLL) {
        const int S = split_slices(quads);
        if (training) EE_LAUNCH(bn_split_stats_kernel, split_grid(C, S), dim3(SPLIT_NT), 0, st, x, workspace, s, S);
        dispatch(relu != 0, residual != nullptr, [&](auto R, auto Q) {
            launch_fwd_args(bn_split_apply_kernel<decltype(R)::value, decltype(Q)::value>, split_grid(C, S), dim3(SPLIT_NT), st, a,
                            static_cast<const float *>(workspace), s, S);
        });
    } else {
        dispatch(vec, big, [&](auto V, auto G) { launch_fwd<decltype(G)::value ? 1024 : 256, decltype(V)::value ? 4 : 1>(relu != 0, st, a, s); });
    }
    return launch_status();
}

EE_API int ee_bn_act_bwd2_f32(const float *dy, const float *dy2, const float *y, const float *x, const float *gamma, const float *beta, const float *save_mean,
                             const float *save_invstd, const float *running_mean, const float *running_var, float eps, int training, int relu,
                             float *dx, float *dresidual, float *dgamma, float *dbeta, float *workspace, int B, int C, int HW, void *stream) {
    int status;  // y == NULL with relu: the mask is recomputed from x, gamma, beta (no residual branch: the caller's promise)
    if (bn_args_settled(B, C, HW, dy && x, training, save_mean, save_invstd, running_mean, running_var, status)) return status;
    const BnShape s{B, C, HW};
    const BwdArgs a{dy, dy2, y, x, beta, gamma, save_mean, save_invstd, running_mean, running_var, eps, training, dx, dresidual, dgamma, dbeta};
    const bool vec = (HW % 4 == 0) && al16(dy) && al16(dy2) && al16(y) && al16(x) && al16(dx) && al16(dresidual);
    const bool big = static_cast<int64_t>(B) * HW >= 16384;
    const int64_t quads = static_cast<int64_t>(B) * (HW / 4), numel = static_cast<int64_t>(B) * C * HW;
    hipStream_t st = as_stream(stream);
    const bool cached = with_cached_cfg(vec ? cached_variant(quads, numel) : 0, [&](auto cfg) {
        launch_bwd_cached<decltype(cfg)::NT, decltype(cfg)::MAXV>(relu != 0, st, a, s, nullptr);
    });
    if (cached) {
    } else if (vec && workspace && numel / 4 <= 0x7fffffffLL) {
        const int S = split_slices(quads);
        dispatch(relu != 0, [&](auto R) {
            EE_LAUNCH(bn_split_bwd_partial_kernel<decltype(R)::value>, split_grid(C, S), dim3(SPLIT_NT), 0, st, dy, dy2, y, x, gamma, beta, save_mean,
                      save_invstd, running_mean, running_var, eps, training, workspace, s, S);
            launch_bwd_args(bn_split_bwd_apply_kernel<decltype(R)::value>, split_grid(C, S), dim3(SPLIT_NT), st, a, static_cast<const float *>(workspace), s, S);
        });
    } else {
        dispatch(vec, big, [&](auto V, auto G) { launch_bwd<decltype(G)::value ? 1024 : 256, decltype(V)::value ? 4 : 1>(relu != 0, st, a, s); });
    }
    return launch_status();
}

EE_API int ee_bn_act_bwd_f32(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                             const float *save_invstd, const float *running_mean, const float *running_var, float eps, int training, int relu,
                             float *dx, float *dresidual, float *dgamma, float *dbeta, float *workspace, int B, int C, int HW, void *stream) {
    if (relu && !y) return EE_ERR_NULL;
    return ee_bn_act_bwd2_f32(dy, nullptr, y, x, gamma, nullptr, save_mean, save_invstd, running_mean, running_var, eps, training, relu, dx, dresidual, dgamma,
                              dbeta, workspace, B, C, HW, stream);
}

// ---- the block boundary of a pre-activation network (AWP/Tiny_imagenet/models_tiny_awp/preactresnet.py:28-34): a block ends with a bare
// `out += shortcut`, the next one begins with relu(bn1(out)) and takes the raw sum as its identity input.  One launch each way on the
// register-cached kernels (SUM / ADD flags); shapes they cannot hold are EE_ERR_UNSUPPORTED - the caller adds and calls ee_bn_act_fwd_f32.
EE_API int ee_bn_sum_act_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta, float *running_mean, float *running_var,
                                 float momentum, float eps, int training, int relu, float *sum_out, float *y, float *save_mean, float *save_invstd,
                                 int B, int C, int HW, void *stream) {
    int status;
    if (bn_args_settled(B, C, HW, x && res && y, training, save_mean, save_invstd, running_mean, running_var, status)) return status;
    if (HW % 4 || !al16(x) || !al16(res) || !al16(y) || !al16(sum_out)) return EE_ERR_UNSUPPORTED;
    const BnShape s{B, C, HW};
    const FwdArgs a{x, res, gamma, beta, running_mean, running_var, momentum, eps, training, y, save_mean, save_invstd};
    hipStream_t st = as_stream(stream);
    if (!with_cached_cfg(cached_variant(static_cast<int64_t>(B) * (HW / 4), static_cast<int64_t>(B) * C * HW), [&](auto cfg) {
            launch_fwd_cached<decltype(cfg)::NT, decltype(cfg)::MAXV>(relu != 0, true, st, a, s, sum_out);
        }))
        return EE_ERR_UNSUPPORTED;
    return launch_status();
}

EE_API int ee_bn_sum_act_bwd_f32(const float *dy, const float *dy2, const float *y, const float *s, const float *gamma, const float *beta,
                                 const float *save_mean, const float *save_invstd, const float *running_mean, const float *running_var, float eps,
                                 int training, int relu, const float *ds_add, float *ds, float *dgamma, float *dbeta, int B, int C, int HW,
                                 void *stream) {
    int status;  // y == NULL with relu: the mask is recomputed from s, gamma, beta (the forward's expression)
    if (bn_args_settled(B, C, HW, dy && s && ds, training, save_mean, save_invstd, running_mean, running_var, status)) return status;
    if (HW % 4 || !al16(dy) || !al16(dy2) || !al16(y) || !al16(s) || !al16(ds_add) || !al16(ds)) return EE_ERR_UNSUPPORTED;
    const BnShape sh{B, C, HW};
    const BwdArgs a{dy, dy2, y, s, beta, gamma, save_mean, save_invstd, running_mean, running_var, eps, training, ds, nullptr, dgamma, dbeta};
    hipStream_t st = as_stream(stream);
    if (!with_cached_cfg(cached_variant(static_cast<int64_t>(B) * (HW / 4), static_cast<int64_t>(B) * C * HW), [&](auto cfg) {
            launch_bwd_cached<decltype(cfg)::NT, decltype(cfg)::MAXV>(relu != 0, st, a, sh, ds_add);
        }))
        return EE_ERR_UNSUPPORTED;
    return launch_status();
}

// floats of workspace ee_bn_relu_pool_fwd/bwd_f32 want (statistics partials forward, gradient-sum partials backward); 0 = unsupported shape
EE_API int ee_bn_relu_pool_workspace_floats(int B, int C, int H, int W) {
    PoolShape p;
    if (!pool_shape(B, C, H, W, p)) return 0;
    return C * SPLIT_MAX * 2;
}

static int bn_relu_pool_fwd_impl(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                                 float momentum, float eps, int training, float *y_pool, uint8_t *code, float *x_argmax, float *save_mean,
                                 float *save_invstd, float *workspace, const float *conv_stats, int conv_stats_slices, int B, int C, int H,
                                 int W, void *stream) {
    if (B < 0 || C < 1 || H < 1 || W < 1) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    PoolShape p;
    if (!pool_shape(B, C, H, W, p)) return EE_ERR_UNSUPPORTED;
    if (!x || !y_pool || !code || !workspace) return EE_ERR_NULL;
    if (!stats_ptrs_ok(training, save_mean, save_invstd, running_mean, running_var)) return EE_ERR_NULL;
    if (!aligned16(x)) return EE_ERR_ALIGN;
    hipStream_t st = as_stream(stream);
    const BnShape s{B, C, H * W};
    const int S = split_slices(static_cast<int64_t>(B) * (H * W / 4));
    int mode = training ? 1 : 0;
    const float *wsk = workspace;
    int Sk = S;
    if (training && conv_stats && conv_stats_slices > 0 && conv_stats_slices <= POOL_MERGE_MAX * SPLIT_NT) {
        mode = 3, wsk = conv_stats, Sk = conv_stats_slices;  // merged inside bn_pool_fwd_kernel
    } else if (training && conv_stats && conv_stats_slices > 0) {
        EE_LAUNCH(bn_stats_finalize_kernel, dim3(static_cast<unsigned>(C)), dim3(SPLIT_NT), 0, st, conv_stats, conv_stats_slices, eps, momentum, running_mean,
                  running_var, save_mean, save_invstd);
        mode = 2;
    } else if (training) {
        EE_LAUNCH(bn_split_stats_kernel, dim3(static_cast<unsigned>(C), static_cast<unsigned>(S)), dim3(SPLIT_NT), 0, st, x, workspace, s, S);
    }
    EE_LAUNCH(bn_pool_fwd_kernel, dim3(static_cast<unsigned>(C), static_cast<unsigned>(p.G)), dim3(SPLIT_NT), static_cast<size_t>(H) * W * sizeof(float), st,
              x, gamma, beta, running_mean, running_var, momentum, eps, mode, y_pool, code, save_mean, save_invstd, wsk, p, Sk, x_argmax);
    return launch_status();
}

EE_API int ee_bn_relu_pool_fwd_f32(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                                   float momentum, float eps, int training, float *y_pool, uint8_t *code, float *save_mean,
                                   float *save_invstd, float *workspace, const float *conv_stats, int conv_stats_slices, int B, int C, int H,
                                   int W, void *stream) {
    return bn_relu_pool_fwd_impl(x, gamma, beta, running_mean, running_var, momentum, eps, training, y_pool, code, nullptr, save_mean, save_invstd, workspace,
                                 conv_stats, conv_stats_slices, B, C, H, W, stream);
}

// ... also writing x_argmax [B,C,OH,OW] = x at every window's argmax: ee_bn_relu_pool_bwd_xa_f32 then takes its batch sums from the pooled
// tensors alone (training mode: one pass over the 26 MB map less)
EE_API int ee_bn_relu_pool_fwd_xa_f32(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                                      float momentum, float eps, int training, float *y_pool, uint8_t *code, float *x_argmax, float *save_mean,
                                      float *save_invstd, float *workspace, const float *conv_stats, int conv_stats_slices, int B, int C, int H,
                                      int W, void *stream) {
    if (B > 0 && !x_argmax) return EE_ERR_NULL;
    return bn_relu_pool_fwd_impl(x, gamma, beta, running_mean, running_var, momentum, eps, training, y_pool, code, x_argmax, save_mean, save_invstd, workspace,
                                 conv_stats, conv_stats_slices, B, C, H, W, stream);
}

static int bn_relu_pool_bwd_impl(const float *dy_pool, const float *dy_pool2, const uint8_t *code, const float *x, const float *x_argmax, const float *gamma,
                                 const float *beta, const float *save_mean, const float *save_invstd, const float *running_mean, const float *running_var,
                                 float eps, int training, float *dx, float *dgamma, float *dbeta, float *workspace, int B, int C, int H,
                                 int W, void *stream) {
    if (B < 0 || C < 1 || H < 1 || W < 1) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    PoolShape p;
    if (!pool_shape(B, C, H, W, p)) return EE_ERR_UNSUPPORTED;
    if (!dy_pool || !code || !x || !workspace) return EE_ERR_NULL;
    if (!stats_ptrs_ok(training, save_mean, save_invstd, running_mean, running_var)) return EE_ERR_NULL;
    if (!aligned16(x) || (dx && !aligned16(dx))) return EE_ERR_ALIGN;
    hipStream_t st = as_stream(stream);
    const dim3 grid(static_cast<unsigned>(C), static_cast<unsigned>(p.G)), block(SPLIT_NT);
    const size_t lds = (static_cast<size_t>(p.OH) * p.OW * 5 + 15) / 16 * 16;  // floats + bytes
    // eval mode (running statistics) and no parameter gradients wanted - every iteration of an eval-mode attack: dx = a * dz needs no sums
    p.nosums = (!training && !dgamma && !dbeta) ? 1 : 0;
    if (p.nosums && !dx) return EE_OK;
    if (!p.nosums && training && x_argmax)
        EE_LAUNCH(bn_pool_bwd_sums_pooled_kernel, grid, block, 0, st, dy_pool, dy_pool2, x_argmax, gamma, beta, save_mean, save_invstd, workspace, p);
    else if (!p.nosums)
        EE_LAUNCH((bn_pool_bwd_kernel<false>), grid, block, lds, st, dy_pool, dy_pool2, code, x, gamma, beta, save_mean, save_invstd, running_mean, running_var, eps,
                  training, dx, dgamma, dbeta, workspace, p);
    EE_LAUNCH((bn_pool_bwd_kernel<true>), grid, block, lds, st, dy_pool, dy_pool2, code, x, gamma, beta, save_mean, save_invstd, running_mean, running_var, eps,
              training, dx, dgamma, dbeta, workspace, p);
    return launch_status();
}

EE_API int ee_bn_relu_pool_bwd_f32(const float *dy_pool, const float *dy_pool2, const uint8_t *code, const float *x, const float *gamma, const float *beta,
                                   const float *save_mean, const float *save_invstd, const float *running_mean, const float *running_var,
                                   float eps, int training, float *dx, float *dgamma, float *dbeta, float *workspace, int B, int C, int H,
                                   int W, void *stream) {
    return bn_relu_pool_bwd_impl(dy_pool, dy_pool2, code, x, nullptr, gamma, beta, save_mean, save_invstd, running_mean, running_var, eps, training, dx, dgamma,
                                 dbeta, workspace, B, C, H, W, stream);
}

// ... with x_argmax (ee_bn_relu_pool_fwd_xa_f32; nullable = the form above): training mode takes the batch sums from dy_pool and x_argmax
EE_API int ee_bn_relu_pool_bwd_xa_f32(const float *dy_pool, const float *dy_pool2, const uint8_t *code, const float *x, const float *x_argmax, const float *gamma,
                                      const float *beta, const float *save_mean, const float *save_invstd, const float *running_mean,
                                      const float *running_var, float eps, int training, float *dx, float *dgamma, float *dbeta, float *workspace, int B,
                                      int C, int H, int W, void *stream) {
    return bn_relu_pool_bwd_impl(dy_pool, dy_pool2, code, x, x_argmax, gamma, beta, save_mean, save_invstd, running_mean, running_var, eps, training, dx, dgamma,
                                 dbeta, workspace, B, C, H, W, stream);
}

// 1 when relu(bn_a(xa) + bn_b(xb)) runs as one launch each way (the register-cached variants with 256-lane workgroups), else 0
EE_API int ee_bn_dual_supported(int B, int C, int HW) {
    if (B < 1 || C < 1 || HW < 1 || HW % 4) return 0;
    const int cv = cached_variant(static_cast<int64_t>(B) * (HW / 4), static_cast<int64_t>(B) * C * HW);
    return (cv == 1 || cv == 2) ? 1 : 0;
}

EE_API int ee_bn_dual_fwd_f32(const float *xa, const float *xb, const float *gamma_a, const float *beta_a, float *running_mean_a, float *running_var_a,
                              float momentum_a, float eps_a, float *save_mean_a, float *save_invstd_a, const float *gamma_b, const float *beta_b,
                              float *running_mean_b, float *running_var_b, float momentum_b, float eps_b, float *save_mean_b, float *save_invstd_b,
                              int training, float *y, int B, int C, int HW, void *stream) {
    if (B < 0 || C < 1 || HW < 1) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!ee_bn_dual_supported(B, C, HW)) return EE_ERR_UNSUPPORTED;
    if (!xa || !xb || !y) return EE_ERR_NULL;
    if (training && (!save_mean_a || !save_invstd_a || !save_mean_b || !save_invstd_b)) return EE_ERR_NULL;
    if (!training && (!running_mean_a || !running_var_a || !running_mean_b || !running_var_b)) return EE_ERR_NULL;
    if (!aligned16(xa) || !aligned16(xb) || !aligned16(y)) return EE_ERR_ALIGN;
    const BnShape s{B, C, HW};
    const BnParams pa{gamma_a, beta_a, running_mean_a, running_var_a, momentum_a, eps_a, save_mean_a, save_invstd_a};
    const BnParams pb{gamma_b, beta_b, running_mean_b, running_var_b, momentum_b, eps_b, save_mean_b, save_invstd_b};
    const dim3 grid(static_cast<unsigned>(C)), block(256);
    if (cached_variant(static_cast<int64_t>(B) * (HW / 4), static_cast<int64_t>(B) * C * HW) == 1)
        EE_LAUNCH((bn_dual_fwd_cached_kernel<256, 2>), grid, block, 0, as_stream(stream), xa, xb, pa, pb, training, y, s);
    else
        EE_LAUNCH((bn_dual_fwd_cached_kernel<256, 7>), grid, block, 0, as_stream(stream), xa, xb, pa, pb, training, y, s);
    return launch_status();
}

EE_API int ee_bn_dual_bwd_f32(const float *dy, const float *dy2, const float *y, const float *xa, const float *xb, const float *gamma_a,
                              const float *save_mean_a, const float *save_invstd_a, const float *running_mean_a, const float *running_var_a,
                              float eps_a, const float *gamma_b, const float *save_mean_b, const float *save_invstd_b,
                              const float *running_mean_b, const float *running_var_b, float eps_b, int training, float *dxa, float *dxb,
                              float *dgamma_a, float *dbeta_a, float *dgamma_b, float *dbeta_b, int B, int C, int HW, void *stream) {
    if (B < 0 || C < 1 || HW < 1) return EE_ERR_SHAPE;
    if (B == 0) return EE_OK;
    if (!ee_bn_dual_supported(B, C, HW)) return EE_ERR_UNSUPPORTED;
    if (!dy || !y || !xa || !xb) return EE_ERR_NULL;
    if (training && (!save_mean_a || !save_invstd_a || !save_mean_b || !save_invstd_b)) return EE_ERR_NULL;
    if (!training && (!running_mean_a || !running_var_a || !running_mean_b || !running_var_b)) return EE_ERR_NULL;
    if (!aligned16(dy) || !al16(dy2) || !aligned16(y) || !aligned16(xa) || !aligned16(xb) || !al16(dxa) || !al16(dxb)) return EE_ERR_ALIGN;
    const BnShape s{B, C, HW};
    const BnParams pa{gamma_a, nullptr, const_cast<float *>(running_mean_a), const_cast<float *>(running_var_a), 0.0f, eps_a, const_cast<float *>(save_mean_a),
                      const_cast<float *>(save_invstd_a)};
    const BnParams pb{gamma_b, nullptr, const_cast<float *>(running_mean_b), const_cast<float *>(running_var_b), 0.0f, eps_b, const_cast<float *>(save_mean_b),
                      const_cast<float *>(save_invstd_b)};
    const dim3 grid(static_cast<unsigned>(C)), block(256);
    if (cached_variant(static_cast<int64_t>(B) * (HW / 4), static_cast<int64_t>(B) * C * HW) == 1)
        EE_LAUNCH((bn_dual_bwd_cached_kernel<256, 2>), grid, block, 0, as_stream(stream), dy, dy2, y, xa, xb, pa, pb, training, dxa, dxb, dgamma_a, dbeta_a,
                  dgamma_b, dbeta_b, s);
    else
        EE_LAUNCH((bn_dual_bwd_cached_kernel<256, 7>), grid, block, 0, as_stream(stream), dy, dy2, y, xa, xb, pa, pb, training, dxa, dxb, dgamma_a, dbeta_a,
                  dgamma_b, dbeta_b, s);
    return launch_status();
}

// ---- SyncBatchNorm: the local halves around the two exchanges (see the kernels above; eeadv/syncbn.py does the collectives) ----------
// workspace: ee_syncbn_workspace_floats(B, C, HW) floats.  moments [C][3] = (mean, M2, count) of this rank's batch.
EE_API int ee_syncbn_workspace_floats(int B, int C, int HW) {
    if (B < 1 || C < 1 || HW < 1 || HW % 4) return 0;
    return C * split_slices(static_cast<int64_t>(B) * (HW / 4)) * 2;
}

static int syncbn_check(int B, int C, int HW) {
    if (B < 1 || C < 1 || HW < 1) return EE_ERR_SHAPE;
    if (HW % 4) return EE_ERR_UNSUPPORTED;
    if (static_cast<int64_t>(B) * C * HW / 4 > 0x7fffffffLL) return EE_ERR_SHAPE;
    return EE_OK;
}

EE_API int ee_syncbn_stats_f32(const float *x, float *workspace, float *moments, int B, int C, int HW, void *stream) {
    if (const int e = syncbn_check(B, C, HW)) return e;
    if (!x || !workspace || !moments) return EE_ERR_NULL;
    if (!aligned16(x)) return EE_ERR_ALIGN;
    const BnShape s{B, C, HW};
    const int S = split_slices(static_cast<int64_t>(B) * (HW / 4));
    hipStream_t st = as_stream(stream);
    EE_LAUNCH(bn_split_stats_kernel, split_grid(C, S), dim3(SPLIT_NT), 0, st, x, workspace, s, S);
    EE_LAUNCH(bn_moments_kernel, dim3(static_cast<unsigned>((C + 63) / 64)), dim3(64), 0, st, workspace, moments, s, S);
    return launch_status();
}

// all_moments [W][C][3]: every rank's moments in rank order (all_gather).  Writes y, save_mean / save_invstd (the GLOBAL batch's) and
// updates running_* (nullable) with the global count.
EE_API int ee_syncbn_apply_f32(const float *x, const float *residual, const float *gamma, const float *beta, const float *all_moments, int W,
                               float *running_mean, float *running_var, float momentum, float eps, int relu, float *y, float *save_mean,
                               float *save_invstd, int B, int C, int HW, void *stream) {
    if (const int e = syncbn_check(B, C, HW)) return e;
    if (W < 1) return EE_ERR_SHAPE;
    if (!x || !y || !all_moments || !save_mean || !save_invstd) return EE_ERR_NULL;
    if (!aligned16(x) || !aligned16(y) || !al16(residual)) return EE_ERR_ALIGN;
    const BnShape s{B, C, HW};
    const int S = split_slices(static_cast<int64_t>(B) * (HW / 4));
    hipStream_t st = as_stream(stream);
    dispatch(relu != 0, residual != nullptr, [&](auto R, auto Q) {
        EE_LAUNCH((bn_sync_apply_kernel<decltype(R)::value, decltype(Q)::value>), split_grid(C, S), dim3(SPLIT_NT), 0, st, x, residual, gamma, beta, all_moments,
                  W, running_mean, running_var, momentum, eps, y, save_mean, save_invstd, s, S);
    });
    return launch_status();
}

// sums [C][2] = this rank's (sum dz, sum dz * xhat), dz = relu ? (dy + dy2) * (y > 0) : dy + dy2 (dy2, y nullable as in ee_bn_act_bwd2_f32)
EE_API int ee_syncbn_bwd_sums_f32(const float *dy, const float *dy2, const float *y, const float *x, const float *gamma, const float *beta,
                                  const float *save_mean, const float *save_invstd, int relu, float *workspace, float *sums, int B, int C, int HW,
                                  void *stream) {
    if (const int e = syncbn_check(B, C, HW)) return e;
    if (!dy || !x || !save_mean || !save_invstd || !workspace || !sums) return EE_ERR_NULL;
    if (!aligned16(dy) || !aligned16(x) || !al16(dy2) || !al16(y)) return EE_ERR_ALIGN;
    const BnShape s{B, C, HW};
    const int S = split_slices(static_cast<int64_t>(B) * (HW / 4));
    hipStream_t st = as_stream(stream);
    dispatch(relu != 0, [&](auto R) {
        EE_LAUNCH(bn_split_bwd_partial_kernel<decltype(R)::value>, split_grid(C, S), dim3(SPLIT_NT), 0, st, dy, dy2, y, x, gamma, beta, save_mean, save_invstd,
                  nullptr, nullptr, 0.0f, 1, workspace, s, S);
    });
    EE_LAUNCH(bn_sums_kernel, dim3(static_cast<unsigned>((C + 63) / 64)), dim3(64), 0, st, workspace, sums, C, S);
    return launch_status();
}

// global_sums [C][2]: the all-reduced sums; n_global: elements per channel over all ranks.  dx and / or dresidual (= dz), nullable.
EE_API int ee_syncbn_bwd_apply_f32(const float *dy, const float *dy2, const float *y, const float *x, const float *gamma, const float *beta,
                                   const float *save_mean, const float *save_invstd, const float *global_sums, double n_global, int relu, float *dx,
                                   float *dresidual, int B, int C, int HW, void *stream) {
    if (const int e = syncbn_check(B, C, HW)) return e;
    if (!dy || !x || !save_mean || !save_invstd || !global_sums) return EE_ERR_NULL;
    if (!(n_global >= 1.0)) return EE_ERR_SHAPE;
    if (!aligned16(dy) || !aligned16(x) || !al16(dy2) || !al16(y) || !al16(dx) || !al16(dresidual)) return EE_ERR_ALIGN;
    if (!dx && !dresidual) return EE_OK;
    const BnShape s{B, C, HW};
    const int S = split_slices(static_cast<int64_t>(B) * (HW / 4));
    hipStream_t st = as_stream(stream);
    dispatch(relu != 0, [&](auto R) {
        EE_LAUNCH(bn_sync_bwd_apply_kernel<decltype(R)::value>, split_grid(C, S), dim3(SPLIT_NT), 0, st, dy, dy2, y, x, beta, gamma, save_mean, save_invstd,
                  global_sums, static_cast<float>(n_global), dx, dresidual, s, S);
    });
    return launch_status();
}
