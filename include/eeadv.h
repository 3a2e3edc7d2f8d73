/*
 * eeadv.h - C ABI of libeeadv.so: the MI355X (gfx950) hot path of Edge-Enhancement adversarial training.
 *
 * The reference (Aiqz/Edge-Enhancement) is pure Python on PyTorch and has no FFI of its own; the
 * "interface" each entry point replaces is therefore the group of ATen launches behind a few lines of
 * utils/attacks.py / utils/core.py, cited per function (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd or a torch ROCm tensor's data_ptr()) unless a
 *     parameter is documented "host"; tensors are dense, row-major NCHW / [B,K];
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued
 *     asynchronously on it, nothing synchronises, so every call is hipGraph-capturable;
 *   - return value: 0 = success, < 0 = EE_ERR_* (argument check failed, nothing was launched),
 *     > 0 = the hipError_t reported by the launch;
 *   - fp32 arithmetic follows the operation order of oracle/ee_oracle.c bit for bit (built with
 *     -ffp-contract=off; IEEE division and square root), including sign(NaN) = sign(0) = 0 and the
 *     0*inf = NaN gradient of the edge filter at zero magnitude.
 */
#ifndef EEADV_H
#define EEADV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EE_OK 0
#define EE_ERR_NULL (-1)        /* a required pointer is NULL */
#define EE_ERR_SHAPE (-2)       /* a size / shape argument is out of range */
#define EE_ERR_UNSUPPORTED (-3) /* valid request this build has no kernel for (e.g. C > 4) */
#define EE_ERR_ALIGN (-4)       /* pointer not aligned to the element size */

/* `path` of the launches that give a sample (or a projection problem) one workgroup of 512 threads: ee_fab_proj_*, ee_fab_start_f32, ee_apgd_step_l2_f32,
 * ee_l1_proj_f32, ee_apgd_step_l1_f32, ee_sqatk_*_l2_f32, ee_sqatk_*_l1_f32.  The two paths return the same bits; a value outside the three: EE_ERR_SHAPE.
 * EE_FAB_PATH_*, EE_APGD_L2_PATH_*, EE_APGD_L1_PATH_* and EE_SQATK_L2_PATH_* below are these. */
#define EE_PATH_AUTO 0      /* resident when a sample has at most 12288 elements, else streaming */
#define EE_PATH_RESIDENT 1  /* a sample stays in registers across all passes; more than 12288 elements: EE_ERR_UNSUPPORTED */
#define EE_PATH_STREAMING 2 /* every pass re-reads its inputs; any size, no scratch tensor */

#define EEADV_ABI_VERSION 1

int ee_abi_version(void);
/* static string for an EE_ERR_* / hipError_t code returned by any entry point */
const char *ee_strerror(int code);
/* name of the device the library would launch on, or NULL (host pointer to a static buffer) */
const char *ee_device_name(void);

/* ---------------------------------------------------------------------------------------------
 * PGD / FGSM / free-AT element-wise updates                              (utils/attacks.py)
 * ------------------------------------------------------------------------------------------- */

/* attacks.py:15-17 (also :42-44, :454-456, :492-494):  x = clamp(x0 + noise, lo, hi).
 * `noise` is caller-supplied (U(-eps,eps) for PGD, 0.001*randn for TRADES/ALP :250,:406 with
 * lo = -inf, hi = +inf because those initialisations are not clamped). */
int ee_pgd_init_f32(float *x, const float *x0, const float *noise, int64_t n, float lo, float hi, void *stream);

/* same, with the noise drawn on the device: Philox4x32-10 keyed by (seed, offset), element i uses
 * counter offset + i/4.  dist 0: U(-scale, scale)  (zeros_like(x).uniform_(-eps, eps), attacks.py:16);
 * dist 1: scale * N(0,1)  (0.001 * randn, attacks.py:250).  Streams differ from torch's generators,
 * so parity tests use ee_pgd_init_f32 with injected noise. */
int ee_pgd_init_rng_f32(float *x, const float *x0, int64_t n, float scale, int dist, uint64_t seed,
                        uint64_t offset, float lo, float hi, void *stream);

/* attacks.py:25-27 (same body :52-54 :82-84 :257-259 :298-300 :318-320 :353-355 :414-416 :466-468
 * :505-507), in place on x:
 *     t = x + dir*alpha*sign(g);  t = max(t, x0 - eps);  t = min(t, x0 + eps);  x = clamp(t, lo, hi)
 * dir = +1 ascent (untargeted), -1 descent (targeted).  16 B of HBM traffic per element. */
int ee_pgd_step_f32(float *x, const float *g, const float *x0, int64_t n, float alpha, float eps, float lo,
                    float hi, int dir, void *stream);

/* attacks.py:389-400 (Trades.PGD_L2), in place on x [B, per_sample]: per sample b
 *     gn = sqrt(mean(g_b^2)) + 1e-8;  t = x_b + step * (g_b / gn);  d = t - x0_b;  dn = sqrt(mean(d^2));
 *     if dn > eps: d *= eps / dn;     x_b = clamp(x0_b + d, lo, hi)
 * (l2_norm is the root of the MEAN of squares, attacks.py:360-366).  The two means are accumulated in double and
 * rounded to fp32 once; ATen's fp32 sum order is not reproduced - results agree to ~1e-7, not bit for bit. */
int ee_l2_step_f32(float *x, const float *g, const float *x0, int64_t B, int64_t per_sample, float step, float eps,
                   float lo, float hi, void *stream);

/* attacks.py:121-126 FGSM:  out = clamp(x + dir*alpha*sign(g), lo, hi)   (no eps projection) */
int ee_fgsm_step_f32(float *out, const float *x, const float *g, int64_t n, float alpha, float lo, float hi,
                     int dir, void *stream);

/* ImageNet/free_imagenet/AT_free_imagenet_ddp.py:289-290:  out = clamp(x + delta, lo, hi) */
int ee_add_clamp_f32(float *out, const float *x, const float *delta, int64_t n, float lo, float hi,
                     void *stream);

/* AT_free_imagenet_ddp.py:305-307:  delta[0:n] = clamp(delta[0:n] + alpha*sign(g), -eps, eps) in place.
 * The reference clamps the whole persistent buffer; rows beyond the batch are unchanged and already
 * inside the box, so touching only the n live elements gives the same buffer. */
int ee_freeat_update_f32(float *delta, const float *g, int64_t n, float alpha, float eps, void *stream);

/* the same update when the caller holds g_in1 = dL/d(in1), in1 = clamp(x + delta, 0, 1) (AT_free_imagenet_ddp.py:289-290):
 * the clamp's gradient mask (0 <= x + delta <= 1) is applied in the kernel, dL/d(delta) never exists as a tensor. */
int ee_freeat_update_masked_f32(float *delta, const float *g_in1, const float *x, int64_t n, float alpha, float eps, void *stream);

/* ---- Fast adversarial training (FGSM from a random start), ee_fastat.hip; ImageNet/fgsm_imagenet/main_fast.py, DESIGN.md section 28 ----
 * Three launches, each one grid-strided sweep: 128-bit accesses when n (per_sample for the third) % 4 == 0 and every float pointer is
 * 16-byte aligned, word by word otherwise - the same bits from both.  Every operation is one f32 rounding in the order written.
 *
 * main_fast.py:224-225, 233-235 - the start of a batch, for i < n:
 *     noise != NULL:  delta[i] = noise[i], copied as bits
 *     noise == NULL:  delta[i] = clamp(0 + (u * (eps - (-eps)) + (-eps)), -eps, eps), u = (word >> 8) * 2^-24 with word = word (i & 3) of the
 *                     Philox4x32-10 call keyed by `seed`, stream 0, counter (step[0] << 32) + (i >> 2): the bits ee_pgd_init_rng_f32(x0 = 0,
 *                     scale = eps, dist 0, seed, offset = step[0] << 32, lo = -eps, hi = eps) writes
 *     in1[i] = clamp(x[i] + delta[i], 0, 1): the bits of ee_add_clamp_f32; a NaN in x or delta gives NaN
 * step is a device uint64[1] (8-byte aligned) that this launch READS and never writes - ee_fastat_ascend_f32 advances it - so a replayed
 * graph draws fresh noise every time; it is not read when noise != NULL and may then be NULL.  The reference redraws its whole persistent
 * buffer (:225); rows of delta beyond n are NOT drawn here: with random_init every step starts by drawing the n live elements, so the
 * rest is never read before it is drawn.  delta may alias noise (the launch is then ee_add_clamp_f32 on the kept noise); delta and in1
 * must not alias x or each other.  n/4 >= 2^32 (group indices (i >> 2) <= (n - 1) / 4 < 2^32 then stay in the counter's low word), eps < 0 or NaN: EE_ERR_SHAPE; a float pointer off 4 bytes, step
 * off 8: EE_ERR_ALIGN; n == 0 launches nothing. */
int ee_fastat_start_f32(float *delta, float *in1, const float *x, const float *noise, int64_t n, float eps, uint64_t seed,
                        const uint64_t *step, void *stream);

/* main_fast.py:246-253 - the noise update and the descend pass's input in one sweep, for i < n, with g = dL/d(in1) of the ascend pass:
 *     s = x[i] + delta[i];  gd = (0 <= s && s <= 1) ? g[i] : 0          the gradient mask of the in-place clamp of :235 (a NaN s masks)
 *     delta[i] = clamp(delta[i] + alpha * sign(gd), -eps, eps)          sign(+-0) = sign(NaN) = 0, sign(+-inf) = +-1
 *     in1[i]   = clamp(x[i] + delta[i], 0, 1)                           with the NEW delta
 * which is ee_freeat_update_masked_f32(delta, g, x, n, alpha, eps) followed by ee_add_clamp_f32(in1, x, delta, n, 0, 1), bit for bit, at
 * 20 B of HBM traffic per element instead of 28.  Afterwards one thread writes step[0] += 1 (a vector store; nothing in this launch
 * reads it); step == NULL: no counter.  in1 is write-only and may alias g (each element is read before it is written); delta and in1
 * must not alias x or each other.  As the free-AT update, only the n live elements of the persistent buffer are touched (:248 clamps all
 * of it; the rest is inside the box already).  n < 0: EE_ERR_SHAPE; a float pointer off 4 bytes, step off 8: EE_ERR_ALIGN; n == 0
 * launches nothing and leaves the counter. */
int ee_fastat_ascend_f32(float *delta, float *in1, const float *g, const float *x, int64_t n, float alpha, float eps, uint64_t *step,
                         void *stream);

/* lib/validation.py:51-57 - the union across PGD restarts, final and x [B, per_sample], logits [B, K], labels [B] (int64):
 *     first != 0:  final[b] = x[b] for every row (:53; logits and labels are not read and may be NULL)
 *     first == 0:  final[b] = x[b] where argmax_k logits[b, k] != labels[b] (:55-57), other rows of final are not written
 * The arg-max is output.max(1)[1]'s: the LOWEST index among equal maxima (+0 and -0 are equal), and a row that holds a NaN gives the index
 * of its FIRST NaN (torch 2.10 on the CPU: torch.tensor([[1., 3., 3.], [0., nan, nan]]).max(1)[1] is [1, 1]; -inf everywhere gives 0).
 * A label outside [0, K) equals no index: the row is copied.  Rows are copied as bits.  One launch: workgroup (b, chunk) finds row b's
 * arg-max for itself and copies its chunk.  final must not alias x (final == x: EE_ERR_SHAPE).  B < 0, per_sample < 1, K < 1 with
 * first == 0: EE_ERR_SHAPE; labels off 8 bytes: EE_ERR_ALIGN; B == 0 launches nothing. */
int ee_fastat_keep_f32(float *final_, const float *x, const float *logits, const int64_t *labels, int64_t B, int64_t K, int64_t per_sample,
                       int first, void *stream);

/* attacks.py:469-479 AVmixup vertex + per-sample mix.  wgt = float64[B] (numpy Beta(1,1) weights):
 *     v = clamp(x0 + (x - x0)*gamma, 0, 1);   out = float(double(x0)*w_b + double(v)*(1 - w_b)) */
int ee_avmix_f32(float *out, const float *x, const float *x0, const double *wgt, int64_t B, int64_t per_sample,
                 float gamma, void *stream);

/* attacks.py:475-478  mixed soft labels, float64 out[B,K]:
 *     y = ls(onehot, l1)*w_b + ls(onehot, l2)*(1 - w_b),  ls(o,f) = o*f + (o-1)*((f-1)/(K-1))  (:444-445, fp32) */
int ee_avmix_labels_f64(double *out, const int64_t *labels, const double *wgt, int64_t B, int64_t K, float lambda1,
                        float lambda2, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Edge filter CannyFilter_step125_1 (utils/core.py:509-585) + To_compare (core.py:329-358)
 *   weights27 = HOST pointer to 27 floats: Gaussian 3x3, Sobel-x 3x3, Sobel-y 3x3, row-major; copied into the kernel arguments
 *   (core.py:524-535; the caller builds them once with get_gaussian_kernel / get_sobel_kernel).
 * ------------------------------------------------------------------------------------------- */

/* forward: x[B,C,H,W] -> edge[B,1,H,W] in {0,1} (fp32).  mag (nullable) receives the gradient
 * magnitude before the alpha mask.  Traffic (C+1)*4 B per pixel. */
int ee_edge125_fwd_f32(const float *x, int B, int C, int H, int W, const float *weights27, float alpha, float high,
                       float *edge, float *mag, void *stream);

/* backward: u = dL/d(edge) [B,1,H,W] -> g_img[B,1,H,W], the map that EVERY input channel of dL/dx
 * receives (the adjoint is identical across channels).  Recomputes the forward from x. */
int ee_edge125_bwd_f32(const float *x, const float *u, int B, int C, int H, int W, const float *weights27,
                       float alpha, float high, float *g_img, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused EE front end   x_in = clamp(x_hfs + w*edge(x), 0, 1)
 *   (Tiny_ImageNet/models_tinyimagenet/resnet_EE.py:176-191, resnet_EE_square.py:187-206,
 *    MNIST/models_mnist/Net2_EE.py:36-49, Net2_EE_square.py:48-63)
 * ------------------------------------------------------------------------------------------- */

/* forward: reads x, x_hfs [B,C,H,W]; writes x_in [B,C,H,W] and gate [B,C,H,W] (uint8: 1 where
 * 0 <= x_hfs + w*edge <= 1, i.e. where clamp passes the gradient).  edge (nullable) [B,1,H,W].
 * 12*C B (+C gate bytes) per pixel. */
int ee_frontend_fwd_f32(const float *x, const float *x_hfs, int B, int C, int H, int W, const float *weights27,
                        float alpha, float high, float w, float *x_in, uint8_t *gate, float *edge, void *stream);

/* backward: g_in = dL/dx_in.  Writes g_hfs = g_in*gate [B,C,H,W] (the gradient entering the
 * low-pass branch) and g_edge [B,1,H,W] (the edge-branch gradient of every channel of x):
 *     u = w * sum_c g_hfs_c ;  g_edge = edge125_bwd(u).                                        */
int ee_frontend_bwd_f32(const float *g_in, const uint8_t *gate, const float *x, int B, int C, int H, int W,
                        const float *weights27, float alpha, float high, float w, float *g_hfs, float *g_edge,
                        void *stream);

/* The same pair keeping the channel-mean Sobel responses gx, gy [B,1,H,W] between the two: the forward writes them (8 more
 * bytes per pixel), the backward then needs neither x nor the blur / Sobel recomputation (about 60 % of the recomputing
 * kernel's instructions) and is bit-identical to ee_frontend_bwd_f32. */
int ee_frontend_fwd_save_f32(const float *x, const float *x_hfs, int B, int C, int H, int W, const float *weights27,
                             float alpha, float high, float w, float *x_in, uint8_t *gate, float *edge, float *gx, float *gy,
                             void *stream);
int ee_frontend_bwd_saved_f32(const float *g_in, const uint8_t *gate, const float *gx, const float *gy, int B, int C, int H,
                              int W, const float *weights27, float alpha, float high, float w, float *g_hfs, float *g_edge,
                              void *stream);

/* ---------------------------------------------------------------------------------------------
 * Full CannyFilter (utils/core.py:148-326): blur, Sobel, magnitude, alpha mask, orientation-quantised non-maximum
 * suppression, straight-through double threshold, hysteresis - the path every model takes (low and high thresholds
 * given, hysteresis=True).  dirs16 = HOST int[16]: (drow, dcol) of the -1 tap of the 8 directional kernels
 * (core.py:87-112; the reference builds them with cv2, the caller passes the derived table -> parity unpinned).
 * ------------------------------------------------------------------------------------------- */

/* forward.  x_in == NULL: edge[B,1,H,W] only.  x_in != NULL: fused front end, x_in = clamp(x_hfs + w*edge, 0, 1) and
 * gate (nullable) as in ee_frontend_fwd_f32; edge then optional. */
int ee_canny_fwd_f32(const float *x, const float *x_hfs, int B, int C, int H, int W, const float *weights27, const int *dirs16,
                     float alpha, float low, float high, float w, float *edge, float *x_in, uint8_t *gate, void *stream);

/* backward.  g_in == NULL: u = dL/d(edge) [B,1,H,W] -> g_img[B,1,H,W].  g_in != NULL (fused front end): u is formed from
 * g_in * gate as in ee_frontend_bwd_f32 and g_hfs = g_in * gate is written too. */
int ee_canny_bwd_f32(const float *x, const float *u, const float *g_in, const uint8_t *gate, int B, int C, int H, int W,
                     const float *weights27, const int *dirs16, float alpha, float low, float high, float w, float *g_img,
                     float *g_hfs, void *stream);

/* last stage of the attack step for EE models, fused: dL/dx = g_lp + g_edge (g_edge broadcast over C),
 * then the PGD update of ee_pgd_step_f32 on x - the gradient itself never reaches HBM.
 * g_lp [B,C,H,W] = gradient arriving through the low-pass branch; g_edge [B,1,H,W]. */
int ee_pgd_step_bcast_f32(float *x, const float *g_lp, const float *g_edge, const float *x0, int B, int C,
                          int64_t hw, float alpha, float eps, float lo, float hi, int dir, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Per-row losses on logits [B,K]  (K <= 65536; one 64-lane wavefront per row)
 *   row_loss: float64[B] per-row values (nullable when only the gradient is wanted)
 *   ee_reduce_rows_f64 folds them in a fixed order -> bit-reproducible scalars.
 * ------------------------------------------------------------------------------------------- */

/* F.cross_entropy incl. label smoothing (attacks.py:23 sum, :255 mean, :89-99 LabelSmoothLoss):
 *     row_loss_b = -sum_k w_bk log_softmax(z_b)_k,  w = smoothing/(K-1) off target, 1-smoothing on it
 *     dz = gscale * (softmax(z) - w)           gscale = 1 ('sum') or 1/B ('mean')
 * A label outside [0, K) gives a NaN row loss and a zero gradient. */
int ee_ce_f32(const float *logits, const int64_t *labels, int B, int K, float smoothing, float gscale,
              double *row_loss, float *dlogits, void *stream);
/* The last two layers of the MNIST classifier and the loss behind them, gradient only (MNIST/models_mnist/Net2.py:27-28 + attacks.py:23):
 * d CrossEntropyLoss(fc2(relu(z1)), labels) / d z1 in one launch.  z1 [B,Hd] = fc1's output, w2 [K,Hd], b2 [K] or NULL, labels [B] ->
 * dz1 [B,Hd] (and the logits [B,K] if logits_out != NULL); gscale = 1 ("sum") or 1/B ("mean").  K <= 64, Hd <= 8192.
 * A label outside [0, K) gives a NaN row loss and a zero gradient: that image's dz1 is zero (its logits are still written). */
int ee_fc_ce_grad_f32(const float *z1, const float *w2, const float *b2, const int64_t *labels, float *dz1, float *logits_out, int B, int Hd,
                      int K, float gscale, void *stream);

/* nn.KLDivLoss('batchmean')(log_softmax(zq), softmax(zp))  (attacks.py:375, :412, :426):
 *     row_loss_b = sum_k p(log p - log q);  dzq = gscale*(q - p);  dzp = gscale*p*((log p - log q) - row_loss_b)
 * dzq / dzp nullable. */
int ee_kl_f32(const float *zq, const float *zp, int B, int K, float gscale, double *row_loss, float *dzq,
              float *dzp, void *stream);

/* -sum_k log_softmax(z)_k * t_k with float64 soft targets (attacks.py:462-463;
 * Tiny_ImageNet/experiments_tinyimagenet.py:292-293): dz (float64, nullable) = gscale*(softmax*sum_k t - t) */
int ee_softce_f64(const float *z, const double *t, int B, int K, double gscale, double *row_loss, double *dz,
                  void *stream);

/* F.mse_loss(a, b) pieces (attacks.py:269): partial[nblk] float64 block sums of (a-b)^2 (nullable),
 * da = gscale*(a - b) (nullable; db = -da).  nblk = ee_mse_num_partials(n). */
int ee_mse_f32(const float *a, const float *b, int64_t n, float gscale, double *partial, float *da, void *stream);
int64_t ee_mse_num_partials(int64_t n);

/* out[0] (float64) = scale * (rows[0] + rows[1] + ...) in a fixed order (single workgroup) */
int ee_reduce_rows_f64(const double *rows, int64_t n, double scale, double *out, void *stream);

/* utils/helper.py:39-55 accuracy / attacks.py:131-132 predict_from_logits:
 * idx[B,k] = sorted top-k class indices (ties: lower index first), correct[k] (int64, zeroed by the
 * call) = number of rows whose label is among the first j+1 indices.  labels nullable; a label outside [0, K) is among no
 * row's indices. */
int ee_topk_i64(const float *logits, const int64_t *labels, int B, int K, int k, int64_t *idx, int64_t *correct,
                void *stream);

/* ---- APGD (Croce & Hein 2020, Linf, one run; EOT: the next section): the per-iteration work around the classifier, ee_apgd.hip ----
 * State of one attack on B samples of per_sample elements each, all in device memory:
 *   x, x_old, x0, g, x_best, g_best, x_best_adv   float [B, per_sample]
 *   fstate  float [4, B]: rows EE_APGD_F_*  (step size, best loss, previous loss, best loss at the last checkpoint)
 *   istate  int   [4, B]: rows EE_APGD_I_*  (loss increases in the window, reduced at the last checkpoint, still robust, flags)
 *   counter int   [1]   : index of the iteration in flight (0-based); ee_apgd_select_f32 advances it
 *   sched   int   [n_iter]: sched[i] = the window length k if a checkpoint closes iteration i, else 0
 * An iteration is step -> classifier forward -> loss -> book -> classifier backward -> select.  No argument changes from one
 * iteration to the next, so a captured graph of one iteration replays for all of them. */
#define EE_APGD_CE 0    /* lse(z) - z_y                                   dlogits = softmax(z) - onehot(y) */
#define EE_APGD_DLR 1   /* -(z_y - z_o) / (z_p1 - z_p3 + 1e-12), o = p2 if p1 == y else p1           (K >= 3) */
#define EE_APGD_DLR_T 2 /* -(z_y - z_t) / (z_p1 - (z_p3 + z_p4)/2 + 1e-12)                           (K >= 4) */
#define EE_APGD_F_STEP 0
#define EE_APGD_F_LOSS_BEST 1
#define EE_APGD_F_PREV 2
#define EE_APGD_F_LOSS_BEST_LAST 3
#define EE_APGD_I_INC 0
#define EE_APGD_I_REDUCED_LAST 1
#define EE_APGD_I_ROBUST 2
#define EE_APGD_I_FLAGS 3
#define EE_APGD_IMPROVED 1 /* flags: the loss beat loss_best -> x_best, g_best take the iterate */
#define EE_APGD_FOOLED 2   /*        the iterate is misclassified -> x_best_adv takes it */
#define EE_APGD_REDUCED 4  /*        the step was halved at a checkpoint -> x, g return to x_best, g_best */

/* The momentum step, in place on x and x_old, with P(v) = clamp(min(max(v, x0 - eps), x0 + eps), 0, 1) and a = 1 when
 * counter[0] == 0, else 0.75:
 *     z = P(x + step[b]*sign(g));  x_new = P((x + (z - x)*a) + (x - x_old)*(1 - a));  x_old = x;  x = x_new
 * b = element / per_sample; sign(NaN) = sign(0) = 0 as in ee_pgd_step_f32.  32 B of HBM traffic per element. */
int ee_apgd_step_f32(float *x, float *x_old, const float *g, const float *x0, const float *step, const int *counter, int64_t B,
                     int64_t per_sample, float eps, void *stream);

/* The step of an APGD run in the L2 threat model (ee_apgd_l2.hip), one launch in the place of ee_apgd_step_f32, in place on x and x_old.
 * Per sample b, with step = step[b], a = 1 when counter[0] == 0, else 0.75, tiny = 1e-12f, every operation rounded once in f32:
 *     ng = ||g||_2                 sg = step / (ng + tiny)
 *     z  = x + g * sg                                       (z = x when ng is not finite: a NaN or Inf gradient takes no gradient step)
 *     d  = z - x0      n1 = ||d||_2      s1 = min(eps, n1) / (n1 + tiny)
 *     z  = clamp(x0 + d * s1, 0, 1)
 *     m  = (x + (z - x) * a) + (x - x_old) * (1 - a)
 *     d  = m - x0      n2 = ||d||_2      s2 = min(eps, n2) / (n2 + tiny)
 *     x_new = clamp(x0 + d * s2, 0, 1);   x_old = x;   x = x_new
 * The rescale followed by the clamp is the published step, not the exact projection onto the intersection of ball and box.  clamp and min
 * propagate NaN.  Each norm is (float) sqrt(S), S the sum of the exact squares in double in an order fixed by per_sample and the launch
 * shape; norms [3, B] receives ng, n1, n2 (required: the trace and the tests read it).  One workgroup per sample; it reads step[b] and
 * counter[0] and advances nothing.  path: EE_APGD_L2_PATH_AUTO picks by size, _RESIDENT keeps a sample's x, x_old, g, x0 in registers
 * across the three reductions (per_sample <= 12288, else EE_ERR_UNSUPPORTED; 24 B of HBM traffic per element), _STREAMING re-reads them
 * (any per_sample; no scratch tensor); the two return the same bits.  16-byte accesses when per_sample % 4 == 0 and x, x_old, g, x0 are
 * 16-byte aligned, element-wise otherwise - the same sums.  eps < 0 or NaN, a path outside the three: EE_ERR_SHAPE.  B == 0 or
 * per_sample == 0 launches nothing. */
#define EE_APGD_L2_PATH_AUTO EE_PATH_AUTO
#define EE_APGD_L2_PATH_RESIDENT EE_PATH_RESIDENT
#define EE_APGD_L2_PATH_STREAMING EE_PATH_STREAMING
int ee_apgd_step_l2_f32(float *x, float *x_old, const float *g, const float *x0, const float *step, const int *counter, float *norms,
                        int64_t B, int64_t per_sample, float eps, int path, void *stream);

/* Per row of logits [B,K]: row_loss[B] (fp32), dlogits[B,K] = d sum_b loss_b / d logits, pred[B] = (p1 == y), where p1, p2, ...
 * are the classes by value descending, ties to the lower index (the order of ee_topk_i64).  kind = EE_APGD_CE / _DLR / _DLR_T;
 * targets [B] is read for EE_APGD_DLR_T only.  K below the kind's minimum: EE_ERR_UNSUPPORTED.  The targeted denominator is formed
 * as ((z_p1 - z_p3) + (z_p1 - z_p4))/2 + 1e-12: the same number without the cancellation of subtracting a rounded sum (the
 * host path of utils/attacks.py keeps z_p1 - (z_p3 + z_p4)/2, so its fp32 loss differs from this one in the last bits).  A label or target outside
 * [0, K) gives that row a NaN loss, a zero gradient and pred = 0. */
int ee_apgd_loss_f32(const float *logits, const int64_t *labels, const int64_t *targets, int B, int K, int kind, float *row_loss,
                     float *dlogits, int *pred, void *stream);

/* The per-sample bookkeeping of one iteration from its losses and pred, one thread per sample, with k = sched[counter[0]]:
 *     robust &= pred;  fooled = !pred;  inc += (loss > f_prev);  f_prev = loss;  improved = loss > loss_best -> loss_best = loss
 *     if k > 0:  reduced = (4*inc <= 3*k) || (!reduced_last && loss_best_last >= loss_best);  reduced_last = reduced;
 *                loss_best_last = loss_best;  inc = 0;  if reduced: step /= 2
 * and writes the three decisions to the flags row of istate.  A counter outside [0, n_iter) is no checkpoint. */
int ee_apgd_book_f32(const float *loss, const int *pred, float *fstate, int *istate, const int *counter, const int *sched, int n_iter,
                     int B, void *stream);

/* The tensor copies the flags [B] ask for, then counter[0] += 1.  Per sample: fooled: x_best_adv = x;  improved: x_best = x,
 * g_best = g;  reduced: x = x_best, g = g_best (x_old stays).  A sample with no flag costs the read of its flag.  B == 0 or
 * per_sample == 0 is no attack: nothing is launched and the counter stays. */
int ee_apgd_select_f32(float *x, float *g, float *x_best, float *g_best, float *x_best_adv, const int *flags, int *counter, int B,
                       int64_t per_sample, void *stream);

/* ---- APGD restarts, ee_apgd_start.hip: the two launches a restart adds, both outside the captured iterations, one
 * workgroup of 512 threads per sample in each.  Both record under EE_K_PGD_STEP.
 *
 * The start point of restart r >= 1, written into x (which must not alias x0): the distribution of the run's own restart 0.  With t a draw
 * of per_sample elements, every operation one f32 rounding in the order written:
 *     EE_FAB_METRIC_LINF  x_i = clamp(x0_i + eps * t_i, 0, 1),  t = 2 u - 1 with u the 24-bit uniform; one pass, no norm
 *     EE_FAB_METRIC_L2    n = (float) sqrt(sum_i t_i^2) - the sum in double in the order of ee_apgd_step_l2_f32's, rounded to float once -,
 *                         s = eps / (n + 1e-12f),  x_i = clamp(x0_i + t_i * s, 0, 1),  t standard normal; n not finite: the row is x0
 *     EE_FAB_METRIC_L1    x_i = x0_i + t_i, NOT clamped,  t standard normal; one pass (the run's ee_l1_proj_f32 follows)
 * noise [B, per_sample] not NULL: t = noise.  noise NULL: t is drawn from Philox4x32-10 keyed by `seed` on stream 16, one call per group of
 * four elements under the counter (b << 32) | (element >> 2) - row b's draw depends on (seed, b, element) alone - the normals being the two
 * Box-Muller pairs of ee_pgd_init_rng_f32 with scale 1.  `path` (EE_PATH_*): the resident path keeps the L2 draw in registers between the
 * norm pass and the write pass, the streaming one reads or draws it again; 128-bit accesses when per_sample % 4 == 0 and x, x0, noise are
 * 16-byte aligned: the same bits from all four.  per_sample >= 1; eps < 0 or NaN, a metric or path outside its three values: EE_ERR_SHAPE;
 * B == 0 launches nothing. */
int ee_apgd_start_f32(float *x, const float *x0, const float *noise, int64_t B, int64_t per_sample, float eps, int metric, uint64_t seed,
                      int path, void *stream);

/* The union across restarts, after restart r's iterations (first != 0: r is restart 0).  robust_run [B] / loss_best_run [B] / x_best_adv are
 * the finished run's (istate row EE_APGD_I_ROBUST, fstate row EE_APGD_F_LOSS_BEST); adv_all [B, per_sample], robust_all [B] (int),
 * loss_all [B] are cumulative.  Sample b:
 *     first:  robust_all = robust_run;  loss_all = loss_best_run;  adv_all[b] = x_best_adv[b] if robust_run == 0
 *     else:   if robust_all != 0 && robust_run == 0: adv_all[b] = x_best_adv[b], robust_all = 0;
 *             loss_all = loss_best_run > loss_all ? loss_best_run : loss_all                      (a NaN never replaces a number)
 * A row that is fooled already is never written again - it keeps the point of the FIRST restart that fooled it; a row never fooled is
 * never written at all.  Rows are copied as bits, 16 bytes at a time where both row starts are 16-byte aligned.  adv_all must not alias
 * x_best_adv.  B == 0 launches nothing. */
int ee_apgd_merge_f32(float *adv_all, int *robust_all, float *loss_all, const float *x_best_adv, const int *robust_run,
                      const float *loss_best_run, int64_t B, int64_t per_sample, int first, void *stream);

/* ---- The perturbation check of an evaluation, ee_pert.hip: one workgroup of 512 threads per sample, one pass over
 * x_adv and x0 [B, per_sample].  Records under EE_K_PGD_STEP.  With d_i = x_adv_i - x0_i, rounded once in f32, sample b gets
 *     norms [B, 3]  max_i |d_i|,  (float) sqrt(sum_i d_i^2),  (float) sum_i |d_i| - both sums in double in the order of
 *                   ee_apgd_step_l2_f32's; a NaN in d (a NaN in either row, or inf - inf) makes all three NaN
 *     range [B, 2]  min_i x_adv_i, max_i x_adv_i with the NaN entries skipped; a row of NaN entries only: (+inf, -inf)
 *     n_nan [B]     the number of NaN entries of x_adv (int)
 * `path` (EE_PATH_*): the resident path loads the sample into registers before it reduces, the streaming one reduces as it reads;
 * 128-bit loads when per_sample % 4 == 0 and x_adv, x0 are 16-byte aligned, word by word otherwise: the same bits from all four.
 * per_sample >= 1; a path outside its three values: EE_ERR_SHAPE; B == 0 launches nothing. */
int ee_pert_check_f32(const float *x_adv, const float *x0, int64_t B, int64_t per_sample, float *norms, float *range, int *n_nan, int path,
                      void *stream);

/* ---- APGD in the L1 threat model (Croce & Hein 2021, "Mind the box"; one run, no momentum, no EOT), ee_apgd_l1.hip ----
 * State next to the APGD run's (x, x0, g, x_best, g_best, x_best_adv, fstate rows EE_APGD_F_STEP / _LOSS_BEST, istate rows
 * EE_APGD_I_ROBUST / _FLAGS, counter, sched), all in device memory:
 *   topk    float [B]   : the share of coordinates the next step moves (starts at 0.2f)
 *   spstate int   [2, B]: row 0 sp_old, the nonzero count of x_best - x0 at the last checkpoint (starts at per_sample); row 1 the count
 *                         the last checkpoint took (for traces and tests)
 *   scal    float [EE_L1_SCAL_ROWS, B]: rows EE_L1_S_*, written by the projection (rows 0-3) and the step (all rows); counts are stored
 *                         as float values, exact below 2^24
 * An iteration is step_l1 -> classifier forward -> ee_apgd_loss_f32 -> book_l1 -> classifier backward -> ee_apgd_select_f32.
 * One workgroup of 512 threads per sample in all three launches. */
#define EE_APGD_L1_PATH_AUTO EE_PATH_AUTO
#define EE_APGD_L1_PATH_RESIDENT EE_PATH_RESIDENT
#define EE_APGD_L1_PATH_STREAMING EE_PATH_STREAMING
#define EE_L1_S_LAMBDA 0 /* the multiplier of the projection (0: the ball is inactive) */
#define EE_L1_S_H0 1     /* h(0) = sum_i (|w_i| - lo_i) as a float; +inf for a sample written as x0 */
#define EE_L1_S_ACTIVE 2 /* |A|, the coordinates strictly between their breakpoints on lambda's segment */
#define EE_L1_S_DIST 3   /* ||z - x0||_1 of what was written (summed in double) */
#define EE_L1_S_TAU 4    /* the step only: the threshold on |g| */
#define EE_L1_S_M 5      /*                the number of coordinates that moved */
#define EE_L1_S_J 6      /*                the rank of tau */
#define EE_L1_SCAL_ROWS 7

/* z = P(u), the Euclidean projection of u onto {z : ||z - x0||_1 <= eps} n [0,1]^D, per sample.  Per coordinate w = u - x0, a = |w|,
 * lo = min(max(0, -min(1 - u, u)), a) (how far u lies outside the box), every f32 operation rounded once:
 *     z = clamp(x0 + sign(w) * (a - min(max(lambda, lo), a)), 0, 1)
 * lambda = 0 when h(0) <= eps, else the root of h(lambda) = sum_i (a_i - min(max(lambda, lo_i), a_i)) = eps: T, the largest float with
 * h(T) > eps, comes from 31 steps over the bit pattern of non-negative floats; on (T, T+] (T+ the next float) the root is
 * (sum_{lo_i > T} (a_i - lo_i) + sum_{lo_i <= T < a_i} a_i - eps) / |A|, rounded to float and kept inside [T, T+]; |A| = 0 takes T+.
 * All sums in double in an order fixed by per_sample and the launch shape.  eps = 0 returns x0 exactly.  A sample whose u - x0 holds a
 * NaN or an Inf is written as x0 (lambda 0, h0 +inf).  x0 outside [0,1] is outside the contract and only loses optimality.  z may be u.
 * scal [>= 4, B] receives rows EE_L1_S_LAMBDA .. _DIST.  Paths, 16-byte accesses and error codes as ee_apgd_step_l2_f32; per_sample above
 * INT32_MAX - 2048 is EE_ERR_SHAPE in the three L1 entry points (a pass counts the padded slots of its last float4 group in an int). */
int ee_l1_proj_f32(float *z, const float *u, const float *x0, float *scal, int64_t B, int64_t per_sample, float eps, int path, void *stream);

/* The step of an L1 run, in place on x: selection, sparse sign step and projection in one launch.  Per sample, D = per_sample:
 *     j   = clamp((int) floorf((1.0f - topk[b]) * (float) D), 0, D - 1)     tau = the j-th smallest |g_i| (0-based, by bit pattern)
 *     m   = #{i : |g_i| >= tau, g_i < 0 or g_i > 0}                         sg  = step[b] / ((float) m + 1e-10f)
 *     u_i = x_i + sg * sign(g_i) where |g_i| >= tau and g_i != 0, else x_i;     x = P(u) as ee_l1_proj_f32
 * Ties at tau all move.  A gradient that holds a NaN or an Inf takes no gradient step (u = x); the projection still runs.
 * scal [EE_L1_SCAL_ROWS, B] receives every row. */
int ee_apgd_step_l1_f32(float *x, const float *g, const float *x0, const float *step, const float *topk, float *scal, int64_t B,
                        int64_t per_sample, float eps, int path, void *stream);

/* The per-sample bookkeeping of one iteration of an L1 run, with k = sched[counter[0]] (a counter outside [0, n_iter) is no checkpoint):
 *     robust &= pred;  fooled = !pred;  improved = loss > loss_best -> loss_best = loss
 *     if k > 0:  sp = #{i : v_i != x0_i}, v = improved ? x : x_best;   reduced = ((float) sp / (float) sp_old) < 0.95f
 *                topk = (float) sp / (float) D / 1.5f;   step = clamp(reduced ? eps : step / 1.5f, eps / 10.0f, eps);   sp_old = sp
 * and writes the three decisions to the flags row of istate (EE_APGD_IMPROVED / _FOOLED / _REDUCED: what ee_apgd_select_f32 reads).
 * fstate [4, B] / istate [4, B] are the APGD run's; only the rows named above are touched. */
int ee_apgd_book_l1_f32(const float *loss, const int *pred, const float *x, const float *x_best, const float *x0, float *fstate,
                        int *istate, float *topk, int *spstate, const int *counter, const int *sched, int n_iter, int64_t B,
                        int64_t per_sample, float eps, void *stream);

/* ---- EOT for APGD (the `rand` version of the public ensemble: each gradient is the mean over E forwards of a randomised defence), ee_eot.hip ----
 * State next to the APGD run's, all in device memory:
 *   g_acc     float  [B, per_sample]  the sum, then the mean, of the E input gradients of one iterate
 *   loss_acc  double [B]              the sum of their row losses, in draw order
 *   loss_mean float  [B]              (float)(loss_acc / E): what ee_apgd_book_f32 reads in an EOT run
 * An iteration is step -> E x (classifier forward -> loss -> classifier backward -> eot_acc) -> book -> select; book sees loss_mean and the
 * LAST draw's pred.  k and E are host values, constants of a captured graph's nodes. */

/* One launch after draw k's backward (0 <= k < E), with inv = 1.0f / E formed in fp32 on the host:
 *     g_acc = (k == 0 ? g : g_acc + g);   if k == E - 1: g_acc = g_acc * inv       (the add is rounded, then the product: never fused)
 *     loss_acc = (k == 0 ? loss : loss_acc + loss) in double;   if k == E - 1: loss_mean = (float)(loss_acc / E)
 * so k == 0 overwrites whatever the accumulators held, E == 1 gives g * 1.0f, and E equal losses give back that loss bit for bit.
 * 16-byte accesses when g_acc and g are 16-byte aligned (a vector may straddle samples; B * per_sample need not be a multiple of 4),
 * element by element otherwise.  12 B of HBM traffic per element (8 B at k == 0).  E < 1 or k outside [0, E): EE_ERR_SHAPE; g_acc == g:
 * EE_ERR_SHAPE; loss_acc 8-byte, the rest 4-byte aligned (EE_ERR_ALIGN).  B == 0 or per_sample == 0 launches nothing. */
int ee_apgd_eot_acc_f32(float *g_acc, const float *g, double *loss_acc, const float *loss, float *loss_mean, int k, int E, int64_t B,
                        int64_t per_sample, void *stream);

/* ---- Square attack (Andriushchenko et al. 2020, Linf, score-based; the schedule of AutoAttack's `standard` version), ee_sqatk.hip ----
 * The ATTACK - not the Add_Square defence (ee_add_square_*, ee_square_draw_f32).  State of one attack on B images [C,H,W], all in
 * device memory:
 *   x0, x_best, x_new  float [B,C,H,W]   the clean images, the best point so far, the proposal the classifier sees
 *   margin_out float [B]  z_y - max_{j != y} z_j of the last forward      margin_min float [B]  the smallest accepted margin (+inf at first)
 *   queries    int   [B]  forwards the sample was active for              flags      int   [B]  1: the last proposal was accepted
 *   counter    int   [1]  index of the next proposal (0-based)            sizes      int   [n_sizes]  window edge of every proposal
 *   seed       int64 [1]  the Philox key of this attack
 * A sample is fooled once margin_min <= 0 and is frozen from then on.  A query is step -> classifier forward on x_new -> margin; no
 * argument changes from one query to the next, so a captured graph of one query replays for all of them.  Randomness is
 * counter-based: r = Philox4x32-10(seed)(ctr, stream_id) with stream_id 11 for windows, ctr = (proposal << 32) | b, and stream_id 12 for
 * the start's stripes, ctr = ((b*C + c) << 32) | (w >> 7): bit (w & 127) of the 128-bit r (x = bits 0..31, y, z, w follow). */

/* The striped start: x_best = x_new = clamp(x0 + (bit ? eps : -eps), 0, 1), one bit per (b, c, w).  C > 32: EE_ERR_UNSUPPORTED. */
int ee_sqatk_init_f32(float *x_best, float *x_new, const float *x0, const int64_t *seed, int B, int C, int H, int W, float eps,
                      void *stream);

/* Per row of logits [B,K], K >= 2, one wavefront per row: margin_out[b] = z_y - max_{j != y} z_j (one fp32 difference: exact); NaN when
 * any logit of the row is NaN or the label is outside [0, K).  If the sample is not fooled (not margin_min <= 0): queries += 1 and the
 * proposal is accepted iff margin < margin_min (never for NaN): margin_min = margin, flags = 1; otherwise flags = 0.  Then counter[0] += 1
 * (this launch never reads it).  B == 0 launches nothing and leaves the counter. */
int ee_sqatk_margin_f32(const float *logits, const int64_t *labels, int B, int K, float *margin_out, float *margin_min, int *queries,
                        int *flags, int *counter, void *stream);

/* Commit and propose, in place.  Per sample: flags[b]: x_best = x_new.  Then, if the sample is not fooled and i = counter[0] is inside
 * [0, n_sizes): with s = sizes[i] (1 <= s <= min(H, W), else no proposal), r = the window draw, vh = umulhi(r.x, H - s + 1),
 * vw = umulhi(r.y, W - s + 1), delta = +-2 eps by bit c of r.z inside rows vh .. vh+s-1, columns vw .. vw+s-1 and 0 outside,
 *     x_new = clamp(min(max(x_best + delta, x0 - eps), x0 + eps), 0, 1).
 * A fooled sample keeps x_new = x_best (after its commit nothing of it is touched again); a counter outside the table (or n_sizes = 0,
 * sizes then nullable) commits only.  128-bit accesses when the three tensors are 16-byte aligned; W and C*H*W need not be multiples
 * of 4.  12 B of HBM traffic per element of a sample whose last proposal was rejected.  C > 32: EE_ERR_UNSUPPORTED. */
int ee_sqatk_step_f32(float *x_best, float *x_new, const float *x0, const int *flags, const float *margin_min, const int *counter,
                      const int *sizes, int n_sizes, const int64_t *seed, int B, int C, int H, int W, float eps, void *stream);

/* ---- Square attack in the L2 threat model (Andriushchenko et al. 2020, Alg. 3), ee_sqatk_l2.hip ----
 * The two launches that stand in the place of ee_sqatk_init_f32 / ee_sqatk_step_f32 in an L2 run; ee_sqatk_margin_f32, the counter, the
 * flags and the query count are shared.  Next to the state above, all in device memory:
 *   eta      float [sum of s*s]  one [s, s] table per distinct window size of the schedule and one for the start's s0: a piecewise-constant
 *                                pattern of unit L2 norm, positive on its top s/2 rows and negative below (eeadv.sqatk.eta forms it in
 *                                float64 and rounds once); the kernels read eta[r][q], or eta[q][r] under a transpose coin
 *   eta_off  int   [n_sizes]     offset in eta of the table of proposal i (its size is sizes[i])
 *   norms    float [3 + 2C, B]   n_img, n_un, n_d, n_w[0..C), n_new[0..C) of the last proposal (zeros for a sample that made none)
 * Draws: window 1 is the Linf window draw (stream 11, ctr = (i << 32) | b: vh, vw from r.x, r.y; bit c of r.z is channel c's sign, bit 0
 * of r.w the transpose coin); window 2 is the same ctr on stream 13 (vh2, vw2 from r.x, r.y; it may overlap window 1); tile k of the start
 * is stream 14, ctr = (b << 32) | k (bit c of r.x channel c's sign, bit 0 of r.y the transpose coin).
 * tiny = 1e-12f; every operation is rounded once in f32; max and clamp propagate NaN.  Each norm is (float) sqrt(S), S the sum of the exact
 * squares in double in an order fixed by C*H*W and the launch shape (one workgroup of 512 threads per sample).  path: EE_SQATK_L2_PATH_AUTO
 * picks by size, _RESIDENT keeps a sample in registers across the reductions (C*H*W <= 12288, else EE_ERR_UNSUPPORTED), _STREAMING
 * re-reads it (any size; no scratch tensor); the two return the same bits.  16-byte accesses when C*H*W % 4 == 0 and x_best, x_new, x0
 * are 16-byte aligned, element-wise otherwise - the same bits.  eps < 0 or NaN, a path outside the three: EE_ERR_SHAPE; C > 32:
 * EE_ERR_UNSUPPORTED.  B == 0 launches nothing.  Both record under EE_K_SQATK_INIT / EE_K_SQATK_STEP. */
#define EE_SQATK_L2_PATH_AUTO EE_PATH_AUTO
#define EE_SQATK_L2_PATH_RESIDENT EE_PATH_RESIDENT
#define EE_SQATK_L2_PATH_STREAMING EE_PATH_STREAMING

/* The tiled start.  eta: the [s0, s0] table; nh = H / s0 by nw = W / s0 tiles from ((H - nh s0) / 2, (W - nw s0) / 2) on, tile k = a * nw + b':
 *     d = +-eta (transposed by the tile's coin) on the tiles, 0 outside;   n0 = ||d||_2;   q = eps / (n0 + tiny)
 *     x_best = x_new = clamp(x0 + d * q, 0, 1)
 * s0 outside [1, min(H, W)]: EE_ERR_SHAPE. */
int ee_sqatk_init_l2_f32(float *x_best, float *x_new, const float *x0, const int64_t *seed, const float *eta, int s0, int B, int C, int H,
                         int W, float eps, int path, void *stream);

/* Commit and propose, in place.  Per sample: flags[b]: x_best = x_new.  Then, if the sample is not fooled and i = counter[0] is inside
 * [0, n_sizes): with s = sizes[i] (1 <= s <= min(H, W), else no proposal), W1 / W2 the two windows and delta = x_best - x0,
 *     n_img = ||delta||_2     n_un = ||delta on W1 u W2||_2 (all channels)     n_w[c] = ||delta[c, W1]||_2
 *     new[c]   = +-eta + delta[c, W1] / (tiny + n_w[c])                          n_new[c] = ||new[c]||_2
 *     scale    = sqrt(max(eps * eps - n_img * n_img, 0) / C + n_un * n_un)
 *     delta[:, W2] = 0;  then  delta[c, W1] = new[c] / (tiny + n_new[c]) * scale  n_d = ||delta||_2
 *     x_new    = clamp(x0 + delta / (tiny + n_d) * eps, 0, 1)
 * A fooled sample keeps x_new = x_best; a counter outside the table (or n_sizes = 0: sizes, eta_off and eta then nullable) commits only.
 * eps = 0 gives x_new = x0; nothing here makes a NaN of finite images. */
int ee_sqatk_step_l2_f32(float *x_best, float *x_new, const float *x0, const int *flags, const float *margin_min, const int *counter,
                         const int *sizes, const int *eta_off, const float *eta, int n_sizes, const int64_t *seed, float *norms, int B,
                         int C, int H, int W, float eps, int path, void *stream);

/* ---- Square attack in the L1 threat model (Croce & Hein 2021, "Mind the box"), ee_sqatk_l1.hip ----
 * The two launches that stand in the place of ee_sqatk_init_f32 / ee_sqatk_step_f32 in an L1 run; ee_sqatk_margin_f32, the counter, the
 * flags and the query count are shared, and eta, eta_off, sizes, the draws (streams 11, 13, 14) and tiny are those of the L2 run above.
 * Two radii: eps, the L1 radius, and eps_p <= eps, the radius every projection uses - the host forms it once as
 * (float) ((double) eps * (1 - 1e-6)); the kernels do not.  P_r(u) is the projection of ee_l1_proj_f32 onto {z : ||z - x0||_1 <= r} n
 * [0,1]^D, the same definition in the same order of sums (its edge rules included: r = 0 returns x0, a non-finite u - x0 writes x0).
 * Next to the state above, all in device memory:
 *   norms    float [2 + 2C, B]   n_img, n_un, n_w[0..C), n_new[0..C) of the last proposal (zeros for a sample that made none)
 *   scal     float [4, B]        rows EE_L1_S_LAMBDA .. _DIST of the launch's projection (zeros for a sample that made no proposal)
 * Each norm is (float) S, S the sum of the |values| in double (exact there) in an order fixed by C*H*W and the launch shape (one workgroup
 * of 512 threads per sample).  Commit, proposal and projection are one launch.  Paths, 16-byte accesses and error codes as the L2 entries;
 * eps or eps_p negative or NaN, eps_p > eps: EE_ERR_SHAPE; C > 32: EE_ERR_UNSUPPORTED; C*H*W above INT32_MAX - 2048: EE_ERR_SHAPE.
 * B == 0 launches nothing.  Both record under EE_K_SQATK_INIT / EE_K_SQATK_STEP. */
#define EE_SQATK_L1_PATH_AUTO EE_PATH_AUTO
#define EE_SQATK_L1_PATH_RESIDENT EE_PATH_RESIDENT
#define EE_SQATK_L1_PATH_STREAMING EE_PATH_STREAMING

/* The tiled start: d the pattern of ee_sqatk_init_l2_f32 bit for bit (not rescaled), u = x0 + d (one addition),
 *     x_best = x_new = P_{eps_p}(u);      scal [4, B] receives the projection's rows.
 * s0 outside [1, min(H, W)]: EE_ERR_SHAPE. */
int ee_sqatk_init_l1_f32(float *x_best, float *x_new, const float *x0, const int64_t *seed, const float *eta, int s0, float *scal, int B,
                         int C, int H, int W, float eps, float eps_p, int path, void *stream);

/* Commit and propose, in place.  Per sample: flags[b]: x_best = x_new.  Then, if the sample is not fooled and i = counter[0] is inside
 * [0, n_sizes): with s = sizes[i] (1 <= s <= min(H, W), else no proposal), W1 / W2 the two windows and delta = x_best - x0,
 *     n_img = ||delta||_1     n_un = ||delta on W1 u W2||_1 (all channels)     n_w[c] = ||delta[c, W1]||_1
 *     new[c]   = +-eta + delta[c, W1] / (tiny + n_w[c])                          n_new[c] = ||new[c]||_1
 *     scale    = max(eps - n_img, 0) / (float) C + n_un
 *     delta[:, W2] = 0;  then  delta[c, W1] = new[c] / (tiny + n_new[c]) * scale
 *     u = x0 + delta (every element);     x_new = P_{eps_p}(u)
 * A fooled sample keeps x_new = x_best and runs no projection (P of a point of the set is not the identity in bits); a counter outside
 * the table (or n_sizes = 0: sizes, eta_off and eta then nullable) commits only.  eps = 0 gives x_new = x0; nothing here makes a NaN of
 * finite images.  With (C + 1) eps <= C*H*W: x_new in [0,1] and ||x_new - x0||_1 <= eps_p + C*H*W * 2^-23. */
int ee_sqatk_step_l1_f32(float *x_best, float *x_new, const float *x0, const int *flags, const float *margin_min, const int *counter,
                         const int *sizes, const int *eta_off, const float *eta, int n_sizes, const int64_t *seed, float *norms,
                         float *scal, int B, int C, int H, int W, float eps, float eps_p, int path, void *stream);

/* ---- FAB-T (Croce & Hein 2020, "Minimally distorted adversarial examples with a fast adaptive boundary attack"; Linf, targeted, one run,
 * eta = 1.05, beta = 0.9, alpha_max = 0.1 - the constants of AutoAttack's `standard` version), ee_fab.hip ----
 * State of one run on B samples of per_sample elements each, all in device memory:
 *   x, x0, adv  float [B, per_sample]   the iterate, the clean input, the closest adversarial point so far
 *   res   float [B]      ||adv - x0||_inf, +inf while none was found      df   float [B]   z_t - z_y at the iterate
 *   scal  float [3, 2B]  rows lambda, sign, ||delta||_inf of the 2B projection problems: problem b projects x[b], problem B + b projects x0[b]
 *   pred  int [B]  the first class of the last logits     flags int [B]  EE_FAB_*     counter int [1]  iterations done
 * An iteration is classifier forward -> diff -> classifier backward (w = d(z_t - z_y)/dx) -> proj -> step -> classifier forward ->
 * commit.  No argument changes from one iteration to the next, so a captured graph of one iteration replays for all of them. */
#define EE_FAB_ADV 1      /* flags: the iterate is misclassified (and no logit of its row is NaN) */
#define EE_FAB_IMPROVED 2 /*        ... and closer to x0 than adv was: adv took it */
#define EE_FAB_PATH_AUTO EE_PATH_AUTO
#define EE_FAB_PATH_RESIDENT EE_PATH_RESIDENT  /* a problem's (|w_i|, r_i) stay in registers */
#define EE_FAB_PATH_STREAMING EE_PATH_STREAMING /* every pass re-reads w and the point */

/* Per row of logits [B,K], K >= 2, one wavefront per row: df[b] = z_t - z_y (one fp32 difference), dlogits[b] = +1 at t, -1 at y (0 at
 * both when t == y), pred[b] = the first class by value descending, ties to the lower index, NaN above everything (the order of
 * ee_topk_i64).  A label or target outside [0, K) gives the row df = NaN and a zero gradient. */
int ee_fab_diff_f32(const float *logits, const int64_t *labels, const int64_t *targets, int B, int K, float *df, float *dlogits, int *pred,
                    void *stream);

/* The box-constrained Linf projection onto the hyperplane <w, .> + b = 0, per problem q of 2B, one workgroup each; scalars only.
 * Problem b: point p = x[b], c = df[b].  Problem B + b: p = x0[b], c = df[b] + sum_i w_i (x0_i - x_i) (a sum of differences, in double).
 * With s = +1 if c >= 0 else -1, v = s w, c' = |c|, room r_i = p_i if v_i > 0, 1 - p_i if v_i < 0, 0 otherwise (never negative) and
 * g(l) = sum_i |v_i| min(l, r_i):  c' >= g(inf): lambda = +inf (infeasible: every moving coordinate goes to its bound);  otherwise lambda =
 * the smallest l with g(l) = c', as the exact solve of the segment of g that contains it ((c' - sum_{r_i <= T} |v_i| r_i) / sum_{r_i > T} |v_i|
 * with T the largest float with g(T) < c', found in 31 steps over the bit pattern; sums in double, one fixed order on both paths: the
 * two paths return the same bits).  out[0][q] = lambda, out[1][q] = s, out[2][q] = min(lambda, max_{v_i != 0} r_i) = ||delta||_inf of
 * delta_i = -sign(v_i) min(lambda, r_i).  A sample whose df or sum |w_i| is not finite or is 0 gets lambda = 0, s = 0, norm = 0 in both
 * problems; c = 0 or not finite in problem B + b alone: lambda = 0, s = +1.  The points are taken to lie in [0,1].  per_sample >= 1, any
 * remainder modulo 4; 128-bit loads when per_sample % 4 == 0 and the tensors are 16-byte aligned. */
int ee_fab_proj_linf_f32(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path, float *out,
                         void *stream);

/* The step, in place on x, from the scalars of ee_fab_proj_linf_f32: with delta1_i = -sign(s1 w_i) min(lambda1, r_i(x)), delta2_i =
 * -sign(s2 w_i) min(lambda2, r_i(x0)) (the rooms as above), a_k = max(norm_k, 1e-8), alpha = min(a1 / (a1 + a2), 0.1):
 *     x = clamp((x + 1.05 delta1) * (1 - alpha) + (x0 + 1.05 delta2) * alpha, 0, 1)
 * in that order, every operation rounded once.  A sample with s1 = 0 (no hyperplane) keeps its x.  16 B of HBM traffic per element. */
int ee_fab_step_f32(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream);

/* The check after the second forward, one workgroup per sample: pred[b] = the first class of logits[b] (order as above); adversarial =
 * pred != y and no logit of the row is NaN (a label outside [0, K) is never adversarial).  If adversarial: n = ||x - x0||_inf; if
 * n < res[b]: adv = x, res[b] = n; then x = x0 + 0.9 (x - x0).  flags[b] = EE_FAB_ADV | EE_FAB_IMPROVED as they apply.  Then
 * counter[0] += 1 (this launch never reads it).  B == 0 or per_sample == 0 launches nothing and leaves the counter. */
int ee_fab_commit_f32(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res, int *pred,
                      int *flags, int *counter, int64_t per_sample, void *stream);

/* ---- FAB-T in the L2 threat model.  The iteration, the state, the flags, the paths and ee_fab_diff_f32 are the
 * ones above; three launches take the place of their Linf siblings and record under the same EE_K_FAB_* families.  res then holds
 * ||adv - x0||_2 and row 2 of scal holds ||delta||_2. */

/* The scalars of the two box-constrained L2 projections of every sample, problems and degenerate-sample rules as in
 * ee_fab_proj_linf_f32: delta = the vector of least ||.||_2 with <w, p + delta> = <w, p> - c and 0 <= p + delta <= 1, which is
 * delta_i = -sign(v_i) min(mu a_i, r_i) (v = s w, a_i = |v_i|, rooms r_i as above; v_i == 0 exactly: delta_i = 0) for the smallest mu >= 0
 * with sum_i a_i min(mu a_i, r_i) = |c|.  out[0][q] = mu (+inf: infeasible, every moving coordinate goes to its bound), out[1][q] = s,
 * out[2][q] = ||delta||_2 = (float) sqrt(sum_i min(mu a_i, r_i)^2) with mu before its rounding to float.  The breakpoint of a
 * coordinate is the f32 quotient r_i / a_i (a denormal a_i: +inf, it never saturates); mu is the exact solve of the segment that the
 * 31-step search over the bit patterns finds.  All sums in double in one fixed order: both paths and both access widths return the
 * same bits.  One workgroup of 512 threads per problem; resident up to 12288 elements, streaming for any size. */
int ee_fab_proj_l2_f32(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path, float *out,
                       void *stream);

/* ee_fab_step_f32 with the deltas of ee_fab_proj_l2_f32: delta_k_i = -sign(s_k w_i) min(mu_k |w_i|, r_i) - the product is one f32
 * multiplication, min propagates NaN - and 0 where w_i == 0 (mu = +inf never meets a zero); a_k, alpha, the convex combination, the clamp
 * and the s1 = 0 rule are unchanged. */
int ee_fab_step_l2_f32(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream);

/* ee_fab_commit_f32 with n = ||x - x0||_2: the squares of the f32 differences summed in double - thread t takes the groups of four
 * elements t, t + 512, ..., then an xor-shuffle tree, then eight partial sums in index order - and n = (float) sqrt(sum).  Vector and
 * element-wise accesses return the same bits.  Everything else is ee_fab_commit_f32's. */
int ee_fab_commit_l2_f32(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res,
                         int *pred, int *flags, int *counter, int64_t per_sample, void *stream);

/* ---- FAB-T in the L1 threat model.  The iteration, the state, the flags, the paths and ee_fab_diff_f32 are the
 * ones above; three launches take the place of their Linf siblings and record under the same EE_K_FAB_* families.  res then holds
 * ||adv - x0||_1, and scal is [4, 2B]: rows theta, sign, ||delta||_1, phi. */

/* The scalars of the two box-constrained L1 projections of every sample, problems and degenerate-sample rules as in
 * ee_fab_proj_linf_f32: delta = a vector of least ||.||_1 with <w, p + delta> = <w, p> - c and 0 <= p + delta <= 1 - a fractional-knapsack
 * fill by descending a_i = |v_i| (v = s w, rooms r_i as above).  With F(T) = sum_{a_i >= T} a_i r_i:  c' > sum_{a_i != 0} a_i r_i
 * (infeasible: every moving coordinate goes to its bound): theta = 0, phi = 1, norm = sum_{a_i != 0} r_i;  otherwise theta = the largest
 * float T with F(T) >= c' (one of the a_i; 31 steps over the bit pattern, no sort), phi = clamp((c' - sum_{a_i > theta} a_i r_i) /
 * sum_{a_i == theta} a_i r_i, 0, 1), and delta_i = -sign(v_i) m_i with m_i = r_i where a_i > theta, phi r_i where a_i == theta (every
 * coordinate tied at theta takes the same fraction of its room), 0 where a_i < theta or v_i == 0.  out[0][q] = theta, out[1][q] = s,
 * out[2][q] = ||delta||_1 = (float)(sum_{a_i > theta} r_i + phi sum_{a_i == theta} r_i) with phi before its rounding to float,
 * out[3][q] = phi.  A sample without a hyperplane: theta = 0, s = 0, norm = 0, phi = 0 in both problems; c = 0 or not finite in problem
 * B + b alone: theta = +inf, s = +1, norm = 0, phi = 0.  All sums in double (the products a_i r_i are exact there) in one fixed order:
 * both paths and both access widths return the same bits.  One workgroup of 512 threads per problem; resident up to 12288 elements,
 * streaming for any size. */
int ee_fab_proj_l1_f32(const float *x, const float *x0, const float *w, const float *df, int64_t B, int64_t per_sample, int path, float *out,
                       void *stream);

/* ee_fab_step_f32 with the deltas of ee_fab_proj_l1_f32, rebuilt from scal [4, 2B]: m_i = r_i above theta_k, phi_k r_i (one f32 product)
 * at theta_k, 0 below it and where w_i is 0 or NaN; a_k, alpha, the convex combination, the clamp and the s1 = 0 rule are unchanged. */
int ee_fab_step_l1_f32(float *x, const float *x0, const float *w, const float *scal, int64_t B, int64_t per_sample, void *stream);

/* ee_fab_commit_f32 with n = ||x - x0||_1: the |f32 differences| summed in double in the order of ee_fab_commit_l2_f32, rounded to float
 * once.  Vector and element-wise accesses return the same bits.  Everything else is ee_fab_commit_f32's. */
int ee_fab_commit_l1_f32(const float *logits, const int64_t *labels, int B, int K, float *x, const float *x0, float *adv, float *res,
                         int *pred, int *flags, int *counter, int64_t per_sample, void *stream);

/* ---- Untargeted FAB (Linf, L2 and L1).  The iteration, the state, the flags, the projections, the step and the
 * commit are the ones above; what changes is where w and df come from: every iteration takes, for each class k = 0 .. K-1 in index order,
 * one backward pass g_k = d(z_k - z_y)/dx off ONE retained forward (its logit gradient from ee_fab_diff_f32 with targets filled with k)
 * and one ee_fab_select_f32, which keeps the class of the closest linearised boundary: afterwards w = g_k*, df = z_k* - z_y.  Two more
 * per-sample buffers: best float [B] (the smallest distance so far), best_k int [B] (its class, -1: none). */
#define EE_FAB_METRIC_LINF 0 /* `metric` of ee_fab_select_f32: the threat model; the distance to a hyperplane is measured in its dual norm */
#define EE_FAB_METRIC_L2 1
#define EE_FAB_METRIC_L1 2

/* One class of the running arg-min, one workgroup of 512 threads per sample.  g [B, per_sample] is the gradient of class k, logits [B, K].
 * n = the dual norm of the row g[b]: sum_i |g_i| (Linf), (float) sqrt(sum_i g_i^2) (L2) - the sums in double, thread t taking the groups
 * of four elements t, t + 512, ..., then an xor-shuffle tree, then eight partial sums in index order, rounded to float once - or max_i |g_i|
 * (L1, exact).  d = z_k - z_y (one fp32 difference), dist = |d| / (1e-12f + n) in float: one add, one divide.  The class is skipped when
 * k == y, when the label lies outside [0, K), or when d or n is not finite or n == 0.  Otherwise, if dist < best[b] strictly: best[b] = dist,
 * best_k[b] = k, df[b] = d and w[b] = g[b] (strict < over ascending k: the lowest class among equal distances).  first != 0 (the launch of
 * class 0) stands in for a reset: best[b] is taken as +inf without being read, and a sample that does not take the class gets best = +inf,
 * best_k = -1, df = 0 (w is left alone: with df = 0 the projections rest, and the step keeps x).  per_sample >= 1, any remainder modulo 4;
 * 128-bit accesses when per_sample % 4 == 0 and g and w are 16-byte aligned, the same bits either way; 0 <= k < K, 2 <= K <= 65536;
 * B == 0 launches nothing.  One streaming pass plus, on improvement, the copy; no `path`.  Records under EE_K_FAB_DIFF. */
int ee_fab_select_f32(const float *g, const float *logits, const int64_t *labels, int k, int metric, int first, int64_t B, int K,
                      int64_t per_sample, float *best, int *best_k, float *w, float *df, void *stream);

/* ---- FAB restarts: the random start of restart r >= 1, one workgroup of 512 threads per sample.  For sample b with
 * the clean row x0[b], the best norm so far res[b] and a draw t of per_sample elements:
 *     m = min(res[b], eps) in float (res = +inf: eps);   n = max_i |t_i| (EE_FAB_METRIC_LINF), (float) sqrt(sum_i t_i^2) (_L2) or
 *     (float) sum_i |t_i| (_L1) - the sums in double in the order of ee_fab_select_f32, rounded to float once;
 *     x_i = clamp(x0_i + ((m * t_i) / n) * 0.5f, 0, 1), every operation one f32 rounding, in this order.
 * n == 0 or not finite: the row is written as x0.  noise [B, per_sample] not NULL: t = noise.  noise NULL: t is drawn from Philox4x32-10
 * keyed by `seed` on stream 15, one call per group of four elements under the counter (b << 32) | (element >> 2) - row b's draw depends
 * on (seed, b, element) alone - t = 2 u - 1 with u the 24-bit uniform (Linf), or the two Box-Muller pairs of ee_pgd_init_rng_f32 with scale 1
 * (L2, L1).  Reads res, writes x (x must not alias x0); `path` as for the projections (EE_PATH_*; the resident path keeps the draw in
 * registers between the norm pass and the write pass, the streaming one reads or draws it again), 128-bit accesses when per_sample % 4 == 0
 * and x, x0, noise are 16-byte aligned: the same bits from all four.  per_sample >= 1; eps < 0 or NaN, a metric or path outside its three
 * values: EE_ERR_SHAPE; B == 0 launches nothing.  Records under EE_K_FAB_STEP. */
int ee_fab_start_f32(float *x, const float *x0, const float *res, const float *noise, int64_t B, int64_t per_sample, float eps, int metric,
                     uint64_t seed, int path, void *stream);

/* CannyFilter_BPDA (utils/core.py:386-505; AWP configs): no alpha mask, NMS by multiplication, thresholds through
 * To_compare (core.py:329-358), hysteresis through To_eq (core.py:361-382).  thresholds given, hysteresis=True.
 *   forward: edge, thin (the thinned magnitude), t2 (the {0, .5, 1} threshold map) [B,1,H,W]; thin / t2 feed the backward.
 *   backward: u = dL/d(edge) -> g_img [B,1,H,W] (the map every input channel receives); g_thin [B,1,H,W] is scratch.
 *   NaN pixels (NaN / inf input only) are not reproduced.  dirs16 as for ee_canny_fwd_f32 (HOST). */
int ee_canny_bpda_fwd_f32(const float *x, int B, int C, int H, int W, const float *weights27, const int *dirs16, float low,
                          float high, float *edge, float *thin, float *t2, void *stream);
int ee_canny_bpda_bwd_f32(const float *x, const float *u, const float *thin, const float *t2, int B, int C, int H, int W,
                          const float *weights27, const int *dirs16, float low, float high, float *g_thin, float *g_img,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * Add_Square (utils/core.py:589-655), element-wise given its random draws
 *   stripe[B,C,W]  = sign(2*rand-1) of core.py:637 ; sq_sign[nq,C] = sign draws of core.py:648 ;
 *   sq_pos[nq] (int64, device: the `.long()` draw) and sq_size[nq] (int32, device) = vh and s of core.py:644-645.
 * ------------------------------------------------------------------------------------------- */
int ee_add_square_fwd_f32(const float *x, int B, int C, int H, int W, float eps, const float *stripe,
                          const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size, int nq, float *out,
                          void *stream);
/* the draws themselves, one launch: stripe[n_stripe] = sign(2u-1) (core.py:637), sq_pos[q] = long((h - sq_size[q]) * u)
 * (core.py:645), sq_sign[nq*C] = sign(2u-1) (core.py:648), u ~ U[0,1) from Philox4x32-10.  state = DEVICE uint64[2]
 * {seed, offset}; the kernel advances the offset itself, so replays of a captured graph draw fresh numbers. */
int ee_square_draw_f32(float *stripe, int64_t n_stripe, int64_t *sq_pos, float *sq_sign, const int32_t *sq_size, int nq,
                       int C, int h, uint64_t *state, void *stream);
/* backward: g_x = g_out * d(out)/d(x), the derivative autograd assigns (ties of max/min split 1/2) */
int ee_add_square_bwd_f32(const float *g_out, const float *x, int B, int C, int H, int W, float eps,
                          const float *stripe, const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size,
                          int nq, float *g_x, void *stream);

/* ---------------------------------------------------------------------------------------------
 * HighFreqSuppress (utils/core.py:15-55) as a fixed real, self-adjoint linear operator, one workgroup per plane
 *   in / out [B,C,H,W], H, W <= 64 (EE_ERR_UNSUPPORTED beyond: callers use the dense two-contraction form there).
 *   tables: DEVICE buffer of ee_hfs_table_floats(H, W, NU, NV) floats built by the host (eeadv/hfs.py):
 *       CwT[NVp][Wp], SwT[NVp][Wp]   cos / sin(2 pi v w / W) for the NV kept half-spectrum column frequencies
 *       ChT[NUp][Hp+4], ShT[NUp][Hp+4], ChN[H][NUp], ShN[H][NUp]   cos / sin(2 pi u h / H) for the NU kept row frequencies
 *       dv[NVp] = kappa_v / W          (NUp, NVp, Hp, Wp: rounded up to multiples of 4, zero padded)
 *   inv_h = 1/H.  The operator equals its own adjoint, so the same call is the backward.
 *   sq_mode 0: y = F(in).  1: y = F(add_square(in))  (core.py:636-655 fused into the load).
 *   2: y = F(in) * d add_square / dx evaluated at sq_x  (the backward of mode 1).  Add_Square draws as in
 *   ee_add_square_fwd_f32.  8 B of HBM traffic per element.
 * ------------------------------------------------------------------------------------------- */
int ee_hfs_table_floats(int H, int W, int NU, int NV);
int ee_hfs_f32(const float *in, float *out, int B, int C, int H, int W, const float *tables, int NU, int NV, float inv_h,
               int sq_mode, const float *sq_x, float eps, const float *stripe, const float *sq_sign, const int64_t *sq_pos,
               const int32_t *sq_size, int nq, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d fused with the residual add and the ReLU that follow it in the reference's ResNet blocks
 * (Tiny_ImageNet/models_tinyimagenet/resnet.py:44-59, :90-110: out = relu(bn(conv(x)) [+ identity])).
 *   x, residual (nullable), y: [B,C,HW] fp32 (NCHW, HW = H*W); gamma / beta (nullable = 1 / 0), running_*: [C].
 *   training != 0: batch statistics (two-pass, biased variance for the output, unbiased for running_var), saved to
 *     save_mean / save_invstd [C]; running_* (nullable) updated with `momentum` as nn.BatchNorm2d does.
 *   training == 0: running statistics.      relu != 0: y = max(., 0) (NaN propagates).
 * backward: dz = relu ? dy * (y > 0) : dy ; dresidual (nullable) = dz ; dgamma / dbeta (nullable) = sum dz*xhat / sum dz ;
 *   dx (nullable) = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) in training mode, gamma*invstd*dz otherwise.
 * Fixed-order reductions: results are bit-reproducible run to run.  One workgroup per channel; a channel too large for one
 * workgroup's registers (B*HW > 28672 values) is split across workgroups in two launches when `workspace` (nullable, DEVICE,
 * ee_bn_workspace_floats(B, C, HW) floats, contents undefined on entry and exit) is given.
 * ------------------------------------------------------------------------------------------- */
int ee_bn_workspace_floats(int B, int C, int HW);
int ee_bn_act_fwd_f32(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                      float *running_var, float momentum, float eps, int training, int relu, float *y, float *save_mean,
                      float *save_invstd, float *workspace, int B, int C, int HW, void *stream);
int ee_bn_act_bwd_f32(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                      const float *save_invstd, const float *running_mean, const float *running_var, float eps, int training,
                      int relu, float *dx, float *dresidual, float *dgamma, float *dbeta, float *workspace, int B, int C, int HW,
                      void *stream);
/* the same with (1) the incoming gradient in two pieces, dy + dy2 (dy2 nullable): a residual block's output feeds the next block's
 * convolution and its identity branch (resnet.py:44-59), and the two gradients are added here, on load, instead of in a launch of
 * their own; (2) y nullable when relu = 1 and the forward had NO residual: the ReLU mask is then recomputed from x, gamma and beta
 * with the forward's expression (the same bits) - one tensor less to read */
int ee_bn_act_bwd2_f32(const float *dy, const float *dy2, const float *y, const float *x, const float *gamma, const float *beta, const float *save_mean,
                       const float *save_invstd, const float *running_mean, const float *running_var, float eps, int training,
                       int relu, float *dx, float *dresidual, float *dgamma, float *dbeta, float *workspace, int B, int C, int HW,
                       void *stream);

/* SyncBatchNorm (ImageNet/experiments_imagenet.py:125, ImageNet/free_imagenet/AT_free_imagenet_ddp.py:149: the reference converts with
 * torch.nn.SyncBatchNorm.convert_sync_batchnorm): the LOCAL halves of a BatchNorm whose batch statistics are those of all ranks' batches.
 * The caller exchanges one small tensor per layer and direction between them (eeadv/syncbn.py over torch.distributed / RCCL):
 *   forward:  ee_syncbn_stats_f32 -> moments [C][3] = this rank's (mean, M2 about it, element count)   | all_gather -> all_moments [W][C][3]
 *             ee_syncbn_apply_f32: merges the W ranks' moments in rank order (Chan's update: the same bits on every rank), writes
 *             save_mean / save_invstd of the global batch, updates running_* (nullable) with the global count (unbiased variance) and
 *             y = [relu]((x - mean) * invstd * gamma + beta [+ residual])
 *   backward: ee_syncbn_bwd_sums_f32 -> sums [C][2] = this rank's (sum dz, sum dz * xhat), which are also its dbeta / dgamma | all_reduce
 *             ee_syncbn_bwd_apply_f32: dx = gamma * invstd * (dz - SUM dz / N - xhat * SUM dz xhat / N) with the global sums, N = n_global;
 *             dresidual = dz.  dy2 / y nullable as in ee_bn_act_bwd2_f32.
 * H*W % 4 == 0, 16-byte aligned tensors; workspace: ee_syncbn_workspace_floats(B, C, HW) floats (0 = unsupported shape). */
int ee_syncbn_workspace_floats(int B, int C, int HW);
int ee_syncbn_stats_f32(const float *x, float *workspace, float *moments, int B, int C, int HW, void *stream);
int ee_syncbn_apply_f32(const float *x, const float *residual, const float *gamma, const float *beta, const float *all_moments, int W,
                        float *running_mean, float *running_var, float momentum, float eps, int relu, float *y, float *save_mean,
                        float *save_invstd, int B, int C, int HW, void *stream);
int ee_syncbn_bwd_sums_f32(const float *dy, const float *dy2, const float *y, const float *x, const float *gamma, const float *beta,
                           const float *save_mean, const float *save_invstd, int relu, float *workspace, float *sums, int B, int C, int HW,
                           void *stream);
int ee_syncbn_bwd_apply_f32(const float *dy, const float *dy2, const float *y, const float *x, const float *gamma, const float *beta,
                            const float *save_mean, const float *save_invstd, const float *global_sums, double n_global, int relu, float *dx,
                            float *dresidual, int B, int C, int HW, void *stream);

/* The end of a residual block with a down-sampling shortcut (resnet.py:54-59 with :137-142): y = relu(bn_a(xa) + bn_b(xb)), bn_a = the
 * block's second BatchNorm on its convolution's output, bn_b = the shortcut's BatchNorm on the 1x1 convolution's output - both per
 * channel, so ONE launch each way instead of two; results bit-identical to ee_bn_act_fwd_f32(xb, relu=0) -> ee_bn_act_fwd_f32(xa,
 * residual, relu=1) and their backwards.  ee_bn_dual_supported: 1 for the shapes it takes (one 256-lane workgroup holds a channel in
 * registers), else use the two calls.  Backward: dy (+ dy2, nullable second piece) -> dxa, dxb (nullable), dgamma / dbeta (nullable). */
int ee_bn_dual_supported(int B, int C, int HW);
int ee_bn_dual_fwd_f32(const float *xa, const float *xb, const float *gamma_a, const float *beta_a, float *running_mean_a, float *running_var_a,
                       float momentum_a, float eps_a, float *save_mean_a, float *save_invstd_a, const float *gamma_b, const float *beta_b,
                       float *running_mean_b, float *running_var_b, float momentum_b, float eps_b, float *save_mean_b, float *save_invstd_b,
                       int training, float *y, int B, int C, int HW, void *stream);
int ee_bn_dual_bwd_f32(const float *dy, const float *dy2, const float *y, const float *xa, const float *xb, const float *gamma_a,
                       const float *save_mean_a, const float *save_invstd_a, const float *running_mean_a, const float *running_var_a,
                       float eps_a, const float *gamma_b, const float *save_mean_b, const float *save_invstd_b,
                       const float *running_mean_b, const float *running_var_b, float eps_b, int training, float *dxa, float *dxb,
                       float *dgamma_a, float *dbeta_a, float *dgamma_b, float *dbeta_b, int B, int C, int HW, void *stream);

/* The block boundary of a pre-activation ResNet (AWP/Tiny_imagenet/models_tiny_awp/preactresnet.py:28-34): s = x + res (one fp32 add per
 * element, as `out += shortcut`), sum_out <- s (nullable), y = [relu](bn(s)) with batch or running statistics; running_* / save_* exactly as
 * ee_bn_act_fwd_f32.  Backward: dz = [y > 0] * (dy [+ dy2]); ds = BN-backward(dz) [+ ds_add] - the gradient of BOTH x and res; dy2 (the
 * second consumer of y), ds_add (what reaches s through the next block's identity branch), dgamma, dbeta nullable; y nullable with relu:
 * the mask is then recomputed from s, gamma and beta with the forward's expression.  One launch each way on the register-cached kernels
 * (B*HW <= 28672, H*W % 4 == 0, 16-byte aligned tensors); other shapes return EE_ERR_UNSUPPORTED before any launch. */
int ee_bn_sum_act_fwd_f32(const float *x, const float *res, const float *gamma, const float *beta, float *running_mean, float *running_var,
                          float momentum, float eps, int training, int relu, float *sum_out, float *y, float *save_mean, float *save_invstd,
                          int B, int C, int HW, void *stream);
int ee_bn_sum_act_bwd_f32(const float *dy, const float *dy2, const float *y, const float *s, const float *gamma, const float *beta,
                          const float *save_mean, const float *save_invstd, const float *running_mean, const float *running_var, float eps,
                          int training, int relu, const float *ds_add, float *ds, float *dgamma, float *dbeta, int B, int C, int HW,
                          void *stream);

/* relu(batch_norm(x)) followed by MaxPool2d(3, stride 2, padding 1) - the ResNet stem (resnet.py:113-117 / :148-150) - without
 * the full-resolution activation: forward x [B,C,H,W] -> y_pool [B,C,OH,OW] + one-byte argmax codes (OH = (H-1)/2+1); backward
 * dy_pool (+ dy_pool2, nullable: the second piece of the gradient, see ee_bn_act_bwd2_f32) + codes + x -> dx [B,C,H,W] (nullable),
 * dgamma, dbeta [C] (nullable).  Values, codes and the pooled-gradient gather equal
 * ee_bn_act_fwd_f32(relu=1) -> ee_maxpool3s2_fwd_f32 and their backwards bit for bit; the gradient sums run over a different
 * partition (dgamma / dbeta / dx agree to rounding).  W % 4 == 0, H*W <= 16000 (else EE_ERR_UNSUPPORTED: use the two calls);
 * workspace: ee_bn_relu_pool_workspace_floats(B, C, H, W) floats (0 = unsupported shape).  conv_stats (nullable): the producing
 * convolution's per-workgroup moments [C][conv_stats_slices][3] (ee_stem7x7s2_fwd_stats_f32); training mode then merges those
 * (Chan's update, fixed order) instead of reading x twice. */
int ee_bn_relu_pool_workspace_floats(int B, int C, int H, int W);
int ee_bn_relu_pool_fwd_f32(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                            float momentum, float eps, int training, float *y_pool, uint8_t *code, float *save_mean,
                            float *save_invstd, float *workspace, const float *conv_stats, int conv_stats_slices, int B, int C, int H,
                            int W, void *stream);
int ee_bn_relu_pool_bwd_f32(const float *dy_pool, const float *dy_pool2, const uint8_t *code, const float *x, const float *gamma, const float *beta,
                            const float *save_mean, const float *save_invstd, const float *running_mean, const float *running_var,
                            float eps, int training, float *dx, float *dgamma, float *dbeta, float *workspace, int B, int C, int H,
                            int W, void *stream);
/* The same pair with one more tensor between them (round 4): the forward also writes x_argmax [B,C,OH,OW] = x at every window's argmax, and
 * the training-mode backward takes its two batch sums from dy_pool and x_argmax alone (a position's masked gradient is the sum of the pooled
 * gradients of the windows whose argmax it is) - one pass over the full-resolution map less.  x_argmax NULL in the backward = the form above.
 * Sums in another order: dgamma / dbeta / dx agree with the form above to rounding. */
int ee_bn_relu_pool_fwd_xa_f32(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                               float momentum, float eps, int training, float *y_pool, uint8_t *code, float *x_argmax, float *save_mean,
                               float *save_invstd, float *workspace, const float *conv_stats, int conv_stats_slices, int B, int C, int H,
                               int W, void *stream);
int ee_bn_relu_pool_bwd_xa_f32(const float *dy_pool, const float *dy_pool2, const uint8_t *code, const float *x, const float *x_argmax, const float *gamma,
                               const float *beta, const float *save_mean, const float *save_invstd, const float *running_mean,
                               const float *running_var, float eps, int training, float *dx, float *dgamma, float *dbeta, float *workspace, int B,
                               int C, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The stem's MaxPool2d(3, stride 2, padding 1) (Tiny_ImageNet/models_tinyimagenet/resnet.py:117), bit-identical to ATen's
 * (first maximum wins, NaN always wins).  x [planes,H,W] -> y, code [planes,OH,OW], OH = (H-1)/2+1; code = 3*kh+kw of the
 * argmax inside its window (one byte).  Backward gathers: dx [planes,H,W] from dy, code.
 * ------------------------------------------------------------------------------------------- */
int ee_maxpool3s2_fwd_f32(const float *x, float *y, uint8_t *code, int planes, int H, int W, void *stream);
int ee_maxpool3s2_bwd_f32(const float *dy, const uint8_t *code, float *dx, int planes, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The shortcut convolution Conv2d(Cin, Cout, kernel_size=1, stride=2, bias=False) of the ResNet blocks
 * (Tiny_ImageNet/models_tinyimagenet/resnet.py:137-142) on the exact-f32 matrix cores.
 *   forward : x [B,Cin,H,W], weight [Cout,Cin] -> y [B,Cout,H/2,W/2]
 *   backward: dy [B,Cout,H/2,W/2] -> dx [B,Cin,H,W] (all of it is written: three of every four pixels are zero)
 *   Cin, Cout, H, W even (EE_ERR_UNSUPPORTED otherwise).  The weight gradient is not provided.
 * ------------------------------------------------------------------------------------------- */
int ee_conv1x1s2_fwd_f32(const float *x, const float *weight, float *y, int B, int Cin, int Cout, int H, int W, void *stream);
int ee_conv1x1s2_bwd_f32(const float *dy, const float *weight, float *dx, int B, int Cin, int Cout, int H, int W, void *stream);

/* Conv2d(3x3, stride 1, padding 1, bias=False) of the residual blocks (resnet.py:26-31) on H x H maps, H = 4, 8 or 16 (ResNet-18 layers 3, 2, 1
 * at 64x64 inputs), forward and backward-data, as Winograd F(2x2, 3x3) around the f32 matrix cores: x [B,KC,H,H], u [16][KC][RC] = the filters
 * in the transform domain, u[4i+j][k][r] = (G g G^T)[i][j] with g = weight[r][k] (forward: KC = Cin, RC = Cout) or g = weight[k][r] rotated by
 * 180 degrees (backward-data: KC = Cout, RC = Cin; x = dy) -> y [B,RC,H,H].  KC % 16 == 0, RC % 32 == 0 (else EE_ERR_UNSUPPORTED).  The weight
 * gradient is not provided.  (Round 3 removed the direct implicit-GEMM kernels ee_conv3x3s1_* / ee_conv3x3s2_* that these and the
 * ee_conv3x3s2_small_* kernels below superseded on every shape of the BASELINE configs.) */
int ee_wino3x3_f32(const float *x, const float *u, float *y, int B, int KC, int RC, int H, void *stream);

/* ---- eval-mode BatchNorm folded into the convolutions (round 4) ---------------------------------------------------------------------------
 * Every validate() pass (experiments_tinyimagenet.py:337 `model.eval()`, then PGD-10/50/100 at :354-358) and the inner loops of ALP / TRADES
 * (utils/attacks.py:249, :405) differentiate the classifier in eval mode: BatchNorm reads its RUNNING statistics and is the per-channel
 * constant map (x - mean) * gamma / sqrt(var + eps) + beta - nothing crosses workgroups, so it needs no launch of its own.  These entry
 * points replace [convolution, BatchNorm(+ residual)(+ ReLU)] (forward) and [BatchNorm/ReLU backward, backward-data convolution] of
 * resnet.py:44-59 by ONE launch each; the expressions and their order are those of ee_bn_act_fwd_f32 / ee_bn_act_bwd2_f32 with
 * training = 0, so the results equal the unfused sequence bit for bit.  mean / var / gamma / beta are [channels] device arrays (gamma / beta
 * may be NULL: 1 / 0).
 *   forward   y = [relu]( (conv3x3(x) - mean) * gamma / sqrt(var + eps) + beta [+ res] )           x [B,Cin,H,H], u = EE_WPREP_WINO_F, res / y [B,Cout,H,H]
 *   backward  dz = (y > 0) * (dy [+ dy2]);  dres <- dz (optional);  dx = conv3x3^T( gamma / sqrt(var + eps) * dz ) [+ dx_add]
 *             dy, dy2, y, dres [B,Cout,H,H]; u_b = EE_WPREP_WINO_B; var / gamma [Cout] (Cout <= 512); dx_add / dx [B,Cin,H,H].  dy2 = the second
 *             piece of a forked output's gradient; dres = the gradient of the block's residual input; dx_add = what reaches the block's input
 *             through the identity branch (one summed gradient then leaves the block). */
int ee_wino3x3_bn_eval_fwd_f32(const float *x, const float *u, const float *mean, const float *var, const float *gamma, const float *beta, float eps,
                               const float *res, int relu, float *y, int B, int Cin, int Cout, int H, void *stream);
int ee_wino3x3_bn_eval_bwd_f32(const float *dy, const float *dy2, const float *y, const float *u_b, const float *var, const float *gamma, float eps,
                               float *dres, const float *dx_add, float *dx, int B, int Cin, int Cout, int H, void *stream);
/* TRAIN-mode BatchNorm with the batch statistics exchanged across the KERNEL BOUNDARY (round 4; resnet.py:44-49: conv1 -> bn1 -> relu ->
 * conv2 inside the attack loop of the training drivers, which runs in train mode - experiments_tinyimagenet.py:234-282).  The producing
 * convolution's output transform writes, next to its raw output, per (channel, image) the plane's (mean, M2) to stats [Cout][B][2]; the
 * consuming convolution's prologue merges the S equal-count partials of each of its reduction channels in a fixed order (bit-reproducible)
 * and stages relu((x - mean) * gamma / sqrt(var + eps) + beta); its first workgroup writes save_mean / save_invstd [Cin] (what
 * ee_bn_act_bwd2_f32(training = 1) reads) and moves running_mean / running_var (may both be NULL) by `momentum` with the unbiased variance,
 * as ee_bn_act_fwd_f32(training = 1) does.  One BatchNorm launch less per residual block and forward pass (10.3 -> 5.2 us,
 * profiles/round4_a_bn_boundary_probe.txt); the statistics are summed in another order than ee_bn_act_fwd_f32's: rounding-level difference.
 * H = 4, 8 or 16; Cin <= 256 for the consumer.  S partials of cnt values each (ee_wino3x3_stats_f32: S = B, cnt = H * H). */
int ee_wino3x3_stats_f32(const float *x, const float *u, float *y, float *stats, int B, int KC, int RC, int H, void *stream);
int ee_wino3x3_bn_train_pre_f32(const float *x, const float *stats, int S, int cnt, const float *gamma, const float *beta, float eps, float momentum,
                                float *running_mean, float *running_var, float *save_mean, float *save_invstd, const float *u, float *y, int B, int KC,
                                int RC, int H, void *stream);
/* The same exchange in the BACKWARD direction (input gradient only; 16x16 maps, <= 128 channels): ee_wino3x3_bwd_sums_f32 is the backward-data
 * convolution of the layer BEHIND the BatchNorm (dy = conv3x3^T(dc) on the backward filter set u_b [16][Cout][Cin]) that also writes per (channel,
 * image) sums [Cin][B][2] = (sum dz, sum dz * xhat), dz = (bn(x) > 0) * dy, from x = the BatchNorm's INPUT and its saved statistics;
 * ee_wino3x3_bn_train_bwd_pre_f32 is the backward-data convolution of the layer in FRONT with the BatchNorm's own backward
 * (gamma * invstd * ((dz - mean dz) - xhat * mean(dz xhat)): ee_bn_act_bwd2_f32 with training = 1, relu = 1 and the mask taken from x)
 * folded into its input staging, the means merged from `sums` (S partials of cnt values) in its prologue. */
int ee_wino3x3_bwd_sums_f32(const float *dc, const float *u_b, const float *x, const float *save_mean, const float *save_invstd, const float *gamma,
                            const float *beta, float *dy, float *sums, int B, int Cin, int Cout, int H, void *stream);
int ee_wino3x3_bn_train_bwd_pre_f32(const float *dy, const float *x, const float *sums, int S, int cnt, const float *save_mean, const float *save_invstd,
                                    const float *gamma, const float *beta, const float *u_b, float *dx, int B, int Cin, int Cout, int H, void *stream);

/* Conv2d(3x3, stride 1, padding 1, bias=False) on a 2x2 map (ResNet-18's layer4 at 64x64 inputs, resnet.py:26-31) as ONE dense product on the
 * f32 matrix cores: every input pixel reaches every output pixel, y[n][(co,p)] = sum x[n][(ci,q)] * w2[(ci,q)][(co,p)], w2 [4 Cin][4 Cout] =
 * EE_WPREP_DENSE_S1 (the backward-data product takes its transpose and Cin / Cout exchanged).  x [B,Cin,2,2] -> y [B,Cout,2,2]; Cin a multiple
 * of 128, Cout of 8.  The *_bn_eval_* forms fold the eval-mode BatchNorm, the residual and the ReLU of the block in exactly as
 * ee_wino3x3_bn_eval_fwd_f32 / _bwd_f32 do (same arguments; w2t [4 Cout][4 Cin] = w2 transposed; Cout <= 512 for the backward). */
int ee_dense2x2_f32(const float *x, const float *w2, float *y, int B, int Cin, int Cout, void *stream);
int ee_dense2x2_bn_eval_fwd_f32(const float *x, const float *w2, const float *mean, const float *var, const float *gamma, const float *beta, float eps,
                                const float *res, int relu, float *y, int B, int Cin, int Cout, void *stream);
int ee_dense2x2_bn_eval_bwd_f32(const float *dy, const float *dy2, const float *y, const float *w2t, const float *var, const float *gamma, float eps,
                                float *dres, const float *dx_add, float *dx, int B, int Cin, int Cout, void *stream);

/* The dot-product non-local product of the feature-denoising block (ImageNet/models_imagenet/resnet_fd.py:126-148 with embed=False,
 * softmax=False) on the f32 matrix cores (ee_fd.hip).  Per sample, X = x[n] as a C x P matrix (P = H * W, rows contiguous):
 *   ee_fd_fwd_f32   f  = scale * X X^T X;  gram [N,d,d], d = min(C, P), receives X X^T (C <= P, the channel form) or X^T X (C > P, the spatial
 *                   form - the reference's rule n_in > H * W), unscaled, for the backward;
 *   ee_fd_bwd_f32   dx = scale * [(M + M^T) X + G D], M = D X^T (channel form) or scale * [D A + X (B + B^T)], B = D^T X (spatial form), D = df,
 *                   G / A = the forward's gram.
 * The long contraction is split over workgroups whose partial d x d tiles meet in `scratch` (ee_fd_scratch_floats(N, C, P) floats, contents
 * undefined on entry and exit) and are added in a fixed order: bit-identical run to run, no atomics; scale multiplies each finished sum once.
 * Up to three launches each; no allocation, no host read.  Shapes: ee_fd_supported(C, P) != 0 - C a multiple of 64, C <= 2048, 1 <= P <= 4096,
 * min(C, P) <= 256 - others EE_ERR_UNSUPPORTED (the scratch query returns 0); N < 0, N > 65535, N*C*P > INT32_MAX, a NaN scale, f == x or
 * dx == x or dx == df: EE_ERR_SHAPE; pointers 4-byte aligned (EE_ERR_ALIGN) - every element is loaded on its own, so 16-byte alignment changes
 * nothing; N == 0 launches nothing. */
int ee_fd_supported(int C, int P);
int64_t ee_fd_scratch_floats(int N, int C, int P);
int ee_fd_fwd_f32(const float *x, float *f, float *gram, float *scratch, int N, int C, int P, float scale, void *stream);
int ee_fd_bwd_f32(const float *x, const float *df, const float *gram, float *dx, float *scratch, int N, int C, int P, float scale, void *stream);

/* The WEIGHT gradient of the same convolution (`loss.backward()` of the training step, experiments_tinyimagenet.py:304-306; resnet.py:26-31) on
 * H x H maps, H = 2, 4, 8 or 16, as Winograd F(3x3, 2x2) around the f32 matrix cores: x [B,Cin,H,H] (the layer's input), dy [B,Cout,H,H] (the
 * gradient of its output) -> dw [Cout,Cin,3,3] (overwritten).  The sum over images and tiles is split over ~256 workgroups whose partial results
 * meet in `workspace` (ee_wrw3x3_workspace_floats(...) floats, contents undefined on entry and exit; 0 = none needed, NULL allowed) and are added
 * in a fixed order: the result is reproducible bit for bit.  Cin, Cout multiples of 32 (else EE_ERR_UNSUPPORTED; the workspace query returns 0). */
int64_t ee_wrw3x3_workspace_floats(int B, int Cin, int Cout, int H);
int ee_wrw3x3_f32(const float *x, const float *dy, float *dw, float *workspace, int B, int Cin, int Cout, int H, void *stream);

/* ... and of the down-sampling blocks' first convolution (3x3 / stride 2 / padding 1 from an H x H map, H = 16, 8 or 4; resnet.py:26-31, :132-137),
 * optionally together with the block's shortcut Conv2d(1x1, stride 2) of the same input (resnet.py:137-142): plain per-tap products on the f32
 * matrix cores, same split + fixed-order sum.  x [B,Cin,H,H], dy3 (and dy1, or NULL) [B,Cout,H/2,H/2] -> dw = [ dw3 [Cout,Cin,3,3] | dw1 [Cout,Cin]
 * (only with dy1) ], overwritten.  Cin, Cout multiples of 32 (else EE_ERR_UNSUPPORTED). */
int64_t ee_wrw3x3s2_workspace_floats(int B, int Cin, int Cout, int H, int with_shortcut);
int ee_wrw3x3s2_f32(const float *x, const float *dy3, const float *dy1, float *dw, float *workspace, int B, int Cin, int Cout, int H, void *stream);

/* ... and of the stem Conv2d(3, 64, 7, stride 2, padding 3, bias=False) (resnet.py:112): x [B,3,H,W], dy [B,64,H/2,W/2] -> dw [64,3,7,7], overwritten;
 * H even, W a multiple of 32 (else EE_ERR_UNSUPPORTED); same split + fixed-order sum. */
int64_t ee_wrw_stem7x7s2_workspace_floats(int B, int H, int W);
int ee_wrw_stem7x7s2_f32(const float *x, const float *dy, float *dw, float *workspace, int B, int H, int W, void *stream);

/* ... and of the 1x1 / stride 1 convolutions of the bottleneck blocks (resnet.py:75-100; ResNet-50 at ImageNet size, BASELINE config 5): both operands
 * are read in their NCHW layout (rows contiguous along the reduction) - x [B,Cin,HW], dy [B,Cout,HW] with HW = H * W pixels, a multiple of 4 ->
 * dw [Cout,Cin], overwritten; Cin, Cout multiples of 64 (else EE_ERR_UNSUPPORTED); same split + fixed-order sum. */
int64_t ee_wrw1x1_workspace_floats(int B, int Cin, int Cout, int HW);
int ee_wrw1x1_f32(const float *x, const float *dy, float *dw, float *workspace, int B, int Cin, int Cout, int HW, void *stream);

/* Conv2d(3x3, stride 2, padding 1, bias=False) between SMALL maps - the first convolution of ResNet-18's layer2 / layer3 / layer4 at 64x64 inputs
 * (resnet.py:26-31, :132-137): H = 16 (16x16 -> 8x8), 8 (8x8 -> 4x4) or 4 (4x4 -> 2x2) - on the f32 matrix cores with the reduction split over a
 * workgroup's wavefronts.  The filters arrive rearranged, w9 [R/32][K/16][9][4][2][16][4] with R = result and K = reduction channels:
 *   forward        x [B,Cin,H,H] -> y [B,Cout,H/2,H/2];  w9[cb][rd][t][q][h][m][k] = weight[32 cb + 16 h + m][16 rd + 4 q + k][t]
 *   backward-data  dy [B,Cout,H/2,H/2] -> dx [B,Cin,H,H] (all of it written, no multiplication by inserted zeros: four parity classes);
 *                  w9[cb][rd][t][q][h][m][k] = weight[16 rd + 4 q + k][32 cb + 16 h + m][t]
 * Cin, Cout multiples of 32 (else EE_ERR_UNSUPPORTED); the weight gradient is not provided. */
int ee_conv3x3s2_small_fwd_f32(const float *x, const float *w9, float *y, int B, int Cin, int Cout, int H, void *stream);
int ee_conv3x3s2_small_bwd_data_f32(const float *dy, const float *w9, float *dx, int B, int Cin, int Cout, int H, void *stream);
/* The same convolution TOGETHER with the shortcut Conv2d(1x1, stride 2, bias=False) of its BasicBlock (resnet.py:50-59, :137-142: both
 * read the block's input, and the 1x1 filter sees exactly the 3x3's centre tap): w10 [R/32][K/16][10][4][2][16][4] = w9 with the 1x1
 * filters as a tenth tap (same index order).  Forward: y3 = conv3x3s2(x), y1 = conv1x1s2(x); backward-data: dx = conv3x3s2^T(dy3) +
 * conv1x1s2^T(dy1) in one pass (the block's input gradient arrives summed). */
int ee_conv3x3s2_pair_fwd_f32(const float *x, const float *w10, float *y3, float *y1, int B, int Cin, int Cout, int H, void *stream);
int ee_conv3x3s2_pair_bwd_data_f32(const float *dy3, const float *dy1, const float *w10, float *dx, int B, int Cin, int Cout, int H, void *stream);
/* ... with the eval-mode BatchNorms behind the two convolutions folded in (see ee_wino3x3_bn_eval_*; resnet.py:50-59, :137-142 under model.eval()):
 *   forward   y3 = relu( bn1(conv3x3s2(x)) ),  y1 = bn_ds(conv1x1s2(x))       (mean3 .. eps3: the block's bn1; mean1 .. eps1: downsample[1])
 *   backward  dx = conv3x3s2^T( gamma3 / sqrt(var3 + eps3) * (y3 > 0) * dy3 ) + conv1x1s2^T( gamma1 / sqrt(var1 + eps1) * dy1 )     (Cout <= 512) */
int ee_conv3x3s2_pair_bn_eval_fwd_f32(const float *x, const float *w10, const float *mean3, const float *var3, const float *gamma3, const float *beta3,
                                      float eps3, const float *mean1, const float *var1, const float *gamma1, const float *beta1, float eps1, float *y3,
                                      float *y1, int B, int Cin, int Cout, int H, void *stream);
int ee_conv3x3s2_pair_bn_eval_bwd_f32(const float *dy3, const float *y3, const float *dy1, const float *w10, const float *var3, const float *gamma3,
                                      float eps3, const float *var1, const float *gamma1, float eps1, float *dx, int B, int Cin, int Cout, int H,
                                      void *stream);
/* ... and, for TRAIN mode, with the statistics of y3 for the BatchNorm behind it (see ee_wino3x3_bn_train_pre_f32): stats [Cout][S][2] = (mean, M2)
 * per result channel and partial - H = 16: S = 2 B half images of 32 values; H = 8: S = B images of 16 values (H = 4: EE_ERR_UNSUPPORTED). */
int ee_conv3x3s2_pair_stats_fwd_f32(const float *x, const float *w10, float *y3, float *y1, float *stats, int B, int Cin, int Cout, int H, void *stream);

/* The filters of the convolution kernels above in the order those kernels read them, from the Conv2d weight [Cout,Cin,3,3] (one launch;
 * the host rebuilds them once per optimiser step, inside the captured update graph):
 *   EE_WPREP_WINO_F / _B   u [16][K][R] for ee_wino3x3_f32, forward (K = Cin, R = Cout) / backward-data (K = Cout, R = Cin, rotated filters)
 *   EE_WPREP_S2M_F / _B    w9 [R/32][K/16][9][4][2][16][4] for ee_conv3x3s2_small_*; EE_WPREP_S2P_F / _B: w10 (10 taps) for ee_conv3x3s2_pair_*,
 *                          w1 [Cout,Cin] = the shortcut's 1x1 filters
 *   EE_WPREP_DENSE_MAP2    [4 Cin][4 Cout]: a 3x3 / stride 1 / padding 1 convolution on a 2x2 map as one dense product (layer 4)
 *   EE_WPREP_WINO_FB       both Winograd sets in one pass over the weight: out = [ u forward [16][Cin][Cout] | u backward-data [16][Cout][Cin] ]
 *                          (2 * 16 * Cin * Cout floats; Cin, Cout multiples of 32), the same values as EE_WPREP_WINO_F / _B */
#define EE_WPREP_WINO_F 0
#define EE_WPREP_WINO_B 1
#define EE_WPREP_S2M_F 2
#define EE_WPREP_S2M_B 3
#define EE_WPREP_S2P_F 4
#define EE_WPREP_S2P_B 5
#define EE_WPREP_DENSE_MAP2 6
#define EE_WPREP_WINO_FB 7
int ee_conv_weight_prep_f32(int kind, const float *w, const float *w1, float *out, int Cout, int Cin, void *stream);
/* ... n of them in ONE launch per 64 items (the captured update of a training step ends with every rearranged copy of the model: 19 launches of
 * ~5 us for ResNet-18 before round 4).  kinds / w / w1 / out / cout / cin: HOST arrays of length n, each item exactly as ee_conv_weight_prep_f32
 * takes it; the same arithmetic, the same bits. */
int ee_conv_weight_prep_batch_f32(int n, const int *kinds, const float *const *w, const float *const *w1, float *const *out, const int *cout, const int *cin,
                                  void *stream);

/* Backward-data of the stem Conv2d(3, K, kernel_size=7, stride=2, padding=3, bias=False) (resnet.py:112-113): the gradient
 * with respect to the image, i.e. the last step of every PGD iteration's backward pass.
 *   dy [B,K,H/2,W/2], weight [K,3,7,7] -> dx [B,3,H,W];  H, W even. */
int ee_stem7x7s2_bwd_data_f32(const float *dy, const float *weight, float *dx, int B, int K, int H, int W, void *stream);
/* The same convolution forward (resnet.py:112-113 / :147): x [B,3,H,W], weight [K,3,7,7] -> y [B,K,H/2,W/2].
 * H, W even, (W/2) % 32 == 0, K % 64 == 0 (else EE_ERR_UNSUPPORTED); weight 16-byte aligned. */
int ee_stem7x7s2_fwd_f32(const float *x, const float *weight, float *y, int B, int K, int H, int W, void *stream);
/* ... and, on the way, the statistics of y for the BatchNorm that follows it (resnet.py:113): stats [K][S][3] = per channel and
 * workgroup (sum, M2 about the tile's own mean, count); ee_stem7x7s2_fwd_stats_floats = K*S*3 (0: unsupported shape).  Hand them to
 * ee_bn_relu_pool_fwd_f32 (conv_stats, conv_stats_slices = S): it then needs no pass over y for its statistics. */
int ee_stem7x7s2_fwd_stats_floats(int B, int K, int H, int W);
int ee_stem7x7s2_fwd_stats_f32(const float *x, const float *weight, float *y, float *stats, int B, int K, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The convolutional half of the MNIST classifier Net_2 (MNIST/models_mnist/Net2.py:13-16), one launch per half each way:
 *   a1 = relu(max_pool2d(conv1(x), 2)),  a2 = relu(max_pool2d(dropmask * conv2(a1), 2))
 *   x [B,1,28,28], w1 [32,1,5,5], b1 [32] (nullable), w2 [64,32,5,5], b2 [64] (nullable), drop [B,64] (nullable: Dropout2d's per-(image,
 *   channel) Bernoulli(keep) draw, 0 or 1, drawn by the caller; the kernels scale by drop / keep, keep = 1 - p).  drop == NULL with
 *   draw_state != NULL (the device-resident {seed, offset, ticket, -} state of ee_square_draw_f32 / ee_chain_fwd_f32): the second kernel makes
 *   the draw itself (Philox4x32-10, stream id 7), writes the mask to drop_out [B,64] for the backward, and its last workgroup advances
 *   the offset - no host-side random launch inside a captured attack iteration
 *   -> a1 [B,32,12,12], a2 [B,64,4,4] and the one-byte argmax codes of the two pools.
 * Backward (input gradient only): da2 [B,64,4,4] -> dx [B,1,28,28] (NULL: skipped); da1 [B,32,12,12] = the gradient of a1, scratch the caller provides.  ReLU backward
 * follows ATen's threshold rule (the gradient passes unless the output is <= 0); pool ties and NaNs follow ATen's max_pool2d. */
int ee_net2_conv_fwd_f32(const float *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *drop, float keep,
                         uint64_t *draw_state, float *drop_out, float *a1, uint8_t *code1, float *a2, uint8_t *code2, int B, void *stream);
int ee_net2_conv_bwd_f32(const float *da2, const float *a2, const uint8_t *code2, const float *drop, float keep, const float *w2,
                         const float *a1, const uint8_t *code1, const float *w1, float *da1, float *dx, int B, void *stream);
/* Parameter gradients of the two halves (a training step's backward): da2 as above, da1 = what ee_net2_conv_bwd_f32 left in its scratch argument
 * -> out = [ dw2 [64,32,5,5] | dw1 [32,1,5,5] | db2 [64] | db1 [32] ] (52096 floats), overwritten; workspace: ee_net2_conv_wrw_workspace_floats(B)
 * floats (0: none needed, NULL allowed).  Groups of ten images are added in order (bit-reproducible). */
int64_t ee_net2_conv_wrw_workspace_floats(int B);
int ee_net2_conv_wrw_f32(const float *x, const float *a1, const uint8_t *code1, const float *da1, const float *a2, const uint8_t *code2, const float *da2,
                         const float *drop, float keep, float *out, float *workspace, int B, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Classifier head: logits = fc(avgpool(feat).view(B,-1)) for a global average pool
 * (Tiny_ImageNet/models_tinyimagenet/resnet.py:157-160).  feat [B,C,HW], weight [K,C], bias [K] (nullable);
 * pooled [B,C] (kept for the weight gradient), logits [B,K].  C <= 4096, K <= 8192 (EE_ERR_UNSUPPORTED beyond).
 * Backward w.r.t. feat: dfeat[b,c,:] = (dlogits[b,:] . weight[:,c]) / HW.
 * ------------------------------------------------------------------------------------------- */
int ee_pool_linear_fwd_f32(const float *feat, const float *weight, const float *bias, float *pooled, float *logits, int B,
                           int C, int HW, int K, void *stream);
int ee_pool_linear_bwd_f32(const float *dlogits, const float *weight, float *dfeat, int B, int C, int HW, int K, void *stream);
/* ... with the cross-entropy gradient formed inside the same launch (the attack loop: attacks.py:23 sum, :255 mean): logits [B,K] as
 * ee_pool_linear_fwd_f32 wrote them, labels [B], gscale = 1 or 1 / B -> dfeat [B,C,HW]; the bits of ee_ce_f32 + ee_pool_linear_bwd_f32.
 * A label outside [0, K) gives a NaN row loss and a zero gradient: that image's dfeat is zero. */
int ee_ce_pool_linear_bwd_f32(const float *logits, const int64_t *labels, float gscale, const float *weight, float *dfeat, int B, int C, int HW,
                              int K, void *stream);

/* HighFreqSuppress for planes up to 256 x 256 (ImageNet 224 x 224, r = 16: utils/core.py:15-55 with cize 224) on the f32 matrix
 * cores, one workgroup per plane, one wavefront per 16-row band (csrc/ee_hfs_mfma.hip).  Same operator, same sq_mode fusions and
 * draw arrays as ee_hfs_f32.  `tables`: ee_hfs_mfma_table_floats(H, W, nu_pad) floats in MFMA fragment order (eeadv/hfs.py:
 * band_tables; the layout is ee_hfs_wide_f32's below at nv_pad = 16); nu_pad = 16 or 32 = the kept row frequencies rounded up.
 * 8 B of HBM traffic per element (12 with sq_mode 2). */
int ee_hfs_mfma_table_floats(int H, int W, int nu_pad);
int ee_hfs_mfma_f32(const float *in, float *out, int B, int C, int H, int W, const float *tables, int nu_pad, int sq_mode,
                    const float *sq_x, float eps, const float *stripe, const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size,
                    int nq, void *stream);
/* ... and for planes past that class, up to 320 x 320 with at most 48 kept row and 32 kept column frequencies (ImageNet/fgsm_imagenet
 * phase 3: 288 x 288, r = 18 keeps 36 and 18): the same kernel with two consecutive 16-row bands per wavefront and [P | Q] up to 64
 * columns wide.  nu_pad = 16, 32 or 48 and nv_pad = 16 or 32 = the kept row / column frequencies rounded
 * up.  `tables`: ee_hfs_wide_table_floats(H, W, nu_pad, nv_pad) floats in MFMA fragment order (eeadv/hfs.py: wide_tables;
 * scripts/chain_emulate.py wide_tables is the layout's specification), with Hp / Wp = H / W rounded up to 16, MT2 = 2 nu_pad / 16,
 * NT = 2 nv_pad / 16 and lane l <-> (l & 15, l >> 4):
 *   t1 [Wp/4][NT][64] | t2 [Hp/16][MT2][4][64] | t3 [Hp/16][MT2][4][64] | t4 [Wp/16][NT][4][64],   16-byte aligned.
 * A size < 1 or a pad outside its set: EE_ERR_SHAPE; H or W > 320: EE_ERR_UNSUPPORTED (both also from ee_hfs_wide_table_floats);
 * B == 0 launches nothing.  Same traffic, same sq_mode fusions, bit-reproducible (the bands are added in band order). */
int ee_hfs_wide_table_floats(int H, int W, int nu_pad, int nv_pad);
int ee_hfs_wide_f32(const float *in, float *out, int B, int C, int H, int W, const float *tables, int nu_pad, int nv_pad, int sq_mode,
                    const float *sq_x, float eps, const float *stripe, const float *sq_sign, const int64_t *sq_pos, const int32_t *sq_size,
                    int nq, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The whole EE front end of one PGD iteration in two launches (csrc/ee_chain.hip): one workgroup per image.
 *   (Tiny_ImageNet/models_tinyimagenet/resnet_EE_square.py:187-206, MNIST/models_mnist/Net2_EE_square.py:48-63,
 *    utils/core.py:15-55, 509-585, 636-655, utils/attacks.py:25-27)
 * Shapes: ee_chain_supported(C, H, W) != 0 - (3,64,64), (1,28,28), (3,32,32), (1,64,64); others EE_ERR_UNSUPPORTED
 * (callers then use ee_hfs_f32 + ee_frontend_* + ee_pgd_step_bcast_f32, same results).
 * `tables`: ee_chain_table_floats(H, W) floats, the constant operands of the low-pass operator in MFMA fragment order
 * (eeadv/hfs.py: chain_tables; scripts/chain_emulate.py is the layout's specification).
 * ------------------------------------------------------------------------------------------- */
int ee_chain_supported(int C, int H, int W);
int ee_chain_table_floats(int H, int W);

/* forward: x[B,C,H,W] -> x_in = clamp(hfs(add_square(x)) + w * edge125(x), 0, 1) [B,C,H,W], gate[B,C,H,W] (uint8: bit 0 = clamp
 * passes the gradient, bits 1-2 = d add_square/dx in {0,1/2,3/4,1} coded 0..3), gx / gy [B,1,H,W] (the Sobel responses the backward
 * starts from), edge (nullable) [B,1,H,W].  square = 0: no Add_Square (resnet_EE.py:176-191).  square = 1: n_queries = 1 with
 * side `sq_size` (core.py:644); the draws (core.py:637, :645, :648) are either injected (stripe_in [B,C,1,W], sq_pos_in [1],
 * sq_sign_in [1,C]: all three) or made in the kernel from Philox4x32-10 with draw_state = uint64[4] {seed, offset, ticket, -}: the
 * element <-> counter mapping is ee_square_draw_f32's, and the last workgroup to finish advances `offset`, so a replayed HIP graph
 * draws fresh numbers.  HBM traffic: read 4C, write 5C + 8 bytes per pixel. */
int ee_chain_fwd_f32(const float *x, int B, int C, int H, int W, const float *tables, const float *weights27, float alpha, float high,
                     float w, int square, float eps, int sq_size, uint64_t *draw_state, const float *stripe_in, const int64_t *sq_pos_in,
                     const float *sq_sign_in, float *x_in, uint8_t *gate, float *gx, float *gy, float *edge, void *stream);

/* backward + update, in place on x: g_in = dL/dx_in [B,C,H,W];
 *     g = dsquare * hfs(gate * g_in) + edge125_adjoint(w * sum_c gate_c * g_in_c)   (NaN where the edge magnitude is 0)
 *     x = clamp(min(max(x + dir*step*sign(g), x0 - eps), x0 + eps), lo, hi)           (attacks.py:25-27)
 * HBM traffic: read 13C + 8, write 4C bytes per pixel. */
int ee_chain_bwd_f32(const float *g_in, const uint8_t *gate, const float *gx, const float *gy, float *x, const float *x0, int B, int C,
                     int H, int W, const float *tables, const float *weights27, float alpha, float high, float w, float step, float eps,
                     float lo, float hi, int dir, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batch assembly from a device-resident dataset split   (utils/data_loader.py: ImageFolder / MNIST
 * + RandomHorizontalFlip + ToTensor, one batch of a DataLoader)
 * ------------------------------------------------------------------------------------------- */

/* data [N,H,W,C] u8 (one split as decoded, HWC), labels [N], idx [B] = the batch's sample ids (a slice of the
 * epoch's order, any order, repeats allowed), flip [N] = per-sample mirror flag of the epoch (nullable: no flip),
 * lut [256] = float(v) / 255 built by the caller (bit-identical to ToTensor by construction):
 *     out[b,c,h,w] = lut[data[idx[b], h, flip[idx[b]] ? W-1-w : w, c]]      out [B,C,H,W] f32
 *     labels_out[b] = labels[idx[b]]                                         labels_out [B]
 * One launch.  C in {1, 3} (EE_ERR_UNSUPPORTED otherwise); out 4-byte aligned (EE_ERR_ALIGN), 16-byte aligned with
 * W % 4 == 0 for the vector path; B == 0 launches nothing.  Precondition: 0 <= idx[b] < N; an id outside that range
 * is not read - its outputs are NaN and its label -1. */
int ee_batch_u8_f32(const uint8_t *data, const int64_t *labels, const int32_t *idx, const uint8_t *flip, const float *lut,
                    long long N, int B, int C, int H, int W, float *out, int64_t *labels_out, void *stream);

/* The same for a split of images of different sizes, each batch sample cropped and resized to S x S (utils/data_loader.py:
 * ImageFolder + RandomResizedCrop(S) + RandomHorizontalFlip + ToTensor).  pixels [nbytes] u8 = the split as one ragged buffer,
 * image n HWC with C = 3 at byte offsets[n], sizes [N,2] = (H_n, W_n), boxes [N,4] = (top, left, h, w) of every sample for this
 * epoch (drawn by the caller), idx / flip / lut / labels as above:
 *     out[b] = lut[ resize(crop(image idx[b], boxes[idx[b]]), S x S) ], mirrored along w when flip[idx[b]]     out [B,3,S,S] f32
 *     labels_out[b] = labels[idx[b]]
 * resize = PIL's 8-bit BILINEAR resample restated: per axis the coefficients of precompute_coeffs in double, rounded to 22-bit
 * fixed point, a horizontal pass over the crop's rows to uint8, then a vertical pass over that to uint8 - the bytes of
 * PIL.Image.crop(box).resize((S, S), BILINEAR), except for a crop with h > 100 w, w >= 2 and S < h, where PIL takes the vertical
 * pass first and some bytes differ by one (eeadv.data.resample_u8 states the condition; RandomResizedCrop never draws one).
 * One launch, one workgroup per (sample, 16 result rows); S <= 4096 (EE_ERR_UNSUPPORTED beyond); out 4-byte aligned
 * (EE_ERR_ALIGN), 16-byte aligned with S % 4 == 0 for the 16-byte stores; B == 0 launches nothing.  Preconditions: 0 <= idx[b] < N,
 * h, w >= 1, the box inside its image and the image inside pixels; a sample that breaks one is not read - its outputs are NaN
 * and its label -1. */
int ee_batch_rrc_u8_f32(const uint8_t *pixels, long long nbytes, const int64_t *offsets, const int32_t *sizes, const int64_t *labels,
                        const int32_t *idx, const int32_t *boxes, const uint8_t *flip, const float *lut, long long N, int B, int S,
                        float *out, int64_t *labels_out, void *stream);

/* The CIFAR-100 train transform on a split of equal-sized images (utils/data_loader.py:30-36: RandomCrop(32, padding=4) +
 * RandomHorizontalFlip() + RandomRotation(15) + ToTensor; the rotation ends in PIL's Image.rotate(angle, NEAREST, fillcolor=0)).
 * data / labels / lut as for ee_batch_u8_f32; per batch position b, drawn by the caller: idx [B] = the sample id, offs [B,2] = (top,
 * left) of the crop in the image zero-padded by `pad` on every side (0 <= top, left <= 2 pad), flip [B] (nullable: no flip) and
 * coef [B,6] = (a0 .. a5), PIL's inverse rotation matrix in 16.16 fixed point with the half-pixel offset folded into a2 and a5
 * (Geometry.c affine_fixed; eeadv.data.aug_coeffs forms it, (65536, 0, 32768, 0, 65536, 32768) is the identity).  Per output pixel:
 *     xin = (a2 + x a0 + y a1) >> 16,  yin = (a5 + x a3 + y a4) >> 16          source pixel in the mirrored crop, 64-bit integers
 *     xs = (flip[b] ? W-1-xin : xin) + left - pad,  ys = yin + top - pad      the same pixel in the image
 *     out[b,c,y,x] = lut[data[idx[b], ys, xs, c]], or 0 when (xin, yin) or (xs, ys) lies outside [0, W) x [0, H)     out [B,C,H,W] f32
 *     labels_out[b] = labels[idx[b]]
 * which is ToTensor(rotate(flip(crop(pad(image))))) bit for bit.  One launch; any C >= 1; out 4-byte aligned (EE_ERR_ALIGN), 16-byte
 * aligned with W % 4 == 0 for the 16-byte stores; B == 0 launches nothing.  idx_host [B] and offs_host [B,2] are HOST copies of idx
 * and offs (the caller drew them on the host): a sample id outside [0, N) or an offset outside [0, 2 pad] in them returns EE_ERR_SHAPE
 * before any launch.  The kernel checks the device arrays again; a sample that breaks a bound there is not read - its outputs are
 * NaN and its label -1. */
int ee_batch_aug_u8_f32(const uint8_t *data, const int64_t *labels, const int32_t *idx, const int32_t *offs, const uint8_t *flip,
                        const int32_t *coef, const float *lut, const int32_t *idx_host, const int32_t *offs_host, long long N, int B, int C,
                        int H, int W, int pad, float *out, int64_t *labels_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sample pools of the survivor-only attack cascade (ee_cascade.hip).
 * A pool is a row store of fixed capacity `cap` on the device: pool_x [cap, D] f32, pool_y [cap] i64 (labels), pool_id [cap] i64
 * (global sample ids), pool_order [cap, K] i64 (the clean-logit class order: the targets of APGD-T and FAB-T) and count [1] i32, the
 * number of rows held.  Rows are copied as bits (NaN payloads survive), with 16-byte accesses where both row starts are 16-byte
 * aligned - decided per row - and word by word otherwise.  Any D >= 1, K >= 1, 1 <= B <= 4096 (EE_ERR_UNSUPPORTED beyond);
 * f32 pointers 4-byte, i64 pointers 8-byte aligned (EE_ERR_ALIGN).  A count outside [0, cap] is read as the nearest bound.  Every
 * loop's trip count follows from the launch shape and D.  The count is read by the copying launches and advanced by a launch of
 * its own after them.
 * ------------------------------------------------------------------------------------------- */
/* Rows b of the batch (x [B,D], y, id [B], order [B,K]) with keep[b] != 0 go behind the count rows already in the pool, in source
 * order: row b lands at count + #{i < b : keep[i] != 0}, counted inside the row's own workgroups; a destination >= cap is not
 * written (the caller keeps count + kept <= cap).  Then count <- min(count + kept, cap).  Two launches. */
int ee_pool_append_f32(const float *x, const int64_t *y, const int64_t *id, const int64_t *order, const uint8_t *keep, int B, long long D,
                       int K, float *pool_x, int64_t *pool_y, int64_t *pool_id, int64_t *pool_order, int32_t *count, long long cap,
                       void *stream);
/* The first B pool rows go to the batch buffers (x [B,D], y, id [B], order [B,K]); a pool holding fewer than B rows fills the rest
 * of the batch with copies of its row 0 (the caller ignores them).  Then rows [B, count) move to the front - the caller pops at
 * count < 2 B, so source and destination rows of that launch are disjoint; cap >= 2 B (EE_ERR_SHAPE) - and
 * count <- min(max(count - B, 0), B).  Three launches. */
int ee_pool_pop_f32(float *pool_x, int64_t *pool_y, int64_t *pool_id, int64_t *pool_order, int32_t *count, long long cap, int B,
                    long long D, int K, float *x, int64_t *y, int64_t *id, int64_t *order, void *stream);
/* After a stage's run on a popped batch: robust [B] (u8, != 0: the stage left the sample correctly classified), id [B], x_adv [B,D]
 * (the stage's result).  For b < n_valid (the rows that are no padding) with 0 <= id[b] < N:
 *     keep[b] = robust[b] != 0;   a broken row writes robust_out[id[b]] = 0, stage_out[id[b]] = stage and, when adv_out [N,D]
 *     is given, adv_out[id[b]] = x_adv[b] (bits).
 * Every other row: keep[b] = 0, nothing else written.  keep [B] u8 is the flag vector of the append into the next pool.  One launch. */
int ee_cascade_resolve_f32(const uint8_t *robust, const int64_t *id, const float *x_adv, int B, int n_valid, long long D, int stage,
                           long long N, uint8_t *robust_out, int32_t *stage_out, float *adv_out, uint8_t *keep, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Optional built-in timing of the last launch of each kernel family (HIP events on `stream`).
 * Off by default; bench.py switches it on outside graph capture to measure kernel durations live.
 * ------------------------------------------------------------------------------------------- */
#define EE_K_PGD_STEP 0 /* ee_pgd_step_f32; also ee_apgd_start_f32 and ee_apgd_merge_f32 (once per restart, outside every captured loop) and ee_pert_check_f32 (once per evaluation) */
#define EE_K_FRONTEND_FWD 1
#define EE_K_FRONTEND_BWD 2
#define EE_K_EDGE_FWD 3
#define EE_K_EDGE_BWD 4
#define EE_K_CE 5
#define EE_K_PGD_STEP_BCAST 6
#define EE_K_EMPTY 7 /* an event pair with nothing in between: the bracket's own cost, see ee_prof_mark_empty */
#define EE_K_HFS 8          /* ee_hfs_f32, sq_mode 0 */
#define EE_K_CHAIN_FWD 9    /* ee_chain_fwd_f32 */
#define EE_K_CHAIN_BWD 10   /* ee_chain_bwd_f32 */
#define EE_K_HFS_SQ_FWD 11  /* ee_hfs_f32, sq_mode 1 (Add_Square on load) */
#define EE_K_HFS_SQ_BWD 12  /* ee_hfs_f32, sq_mode 2 (times d Add_Square / dx on store) */
#define EE_K_SQUARE_DRAW 13 /* ee_square_draw_f32 */
/* 14 - 17: the direct 3x3 kernels removed in round 3 */
#define EE_K_WINO 18        /* ee_wino3x3_f32 (forward and backward-data are the same kernel); work = the convolution's algorithmic flops */
#define EE_K_CONV3S2_FWD 19 /* ee_conv3x3s2_small_fwd_f32; work = flops */
#define EE_K_CONV3S2_BWD 20 /* ee_conv3x3s2_small_bwd_data_f32 */
#define EE_K_WINO_FUSED 21  /* ee_wino3x3_bn_eval_*, ee_wino3x3_stats_f32, ee_wino3x3_bn_train_*, ee_wino3x3_bwd_sums_f32: the same products with the
                             * BatchNorm work of the layer folded into the staging / output stage; work = the convolution's flops only */
#define EE_K_BATCH_AUG 22  /* ee_batch_aug_u8_f32 */
#define EE_K_SQATK_INIT 23   /* ee_sqatk_init_f32 */
#define EE_K_SQATK_MARGIN 24 /* ee_sqatk_margin_f32 */
#define EE_K_SQATK_STEP 25   /* ee_sqatk_step_f32 */
#define EE_K_FAB_DIFF 26     /* ee_fab_diff_f32, ee_fab_select_f32 */
#define EE_K_FAB_PROJ 27     /* ee_fab_proj_linf_f32, ee_fab_proj_l2_f32, ee_fab_proj_l1_f32 */
#define EE_K_FAB_STEP 28     /* ee_fab_step_f32, ee_fab_step_l2_f32, ee_fab_step_l1_f32, ee_fab_start_f32 */
#define EE_K_FAB_COMMIT 29   /* ee_fab_commit_f32, ee_fab_commit_l2_f32, ee_fab_commit_l1_f32 */
#define EE_K_COUNT 30
int ee_prof_enable(int on);
/* records one empty start/stop bracket on `stream` (family EE_K_EMPTY): callers subtract its mean from the other
 * families' means, because a HIP event pair costs ~4-5 us on gfx950 - comparable to the kernels being timed */
int ee_prof_mark_empty(void *stream);
/* synchronises the recorded events and returns accumulated milliseconds / launch count since the last reset */
int ee_prof_read(int kernel_id, double *total_ms, int64_t *launches);
/* sum of the `work` the timed launches of a family declared (floating-point operations for the matrix-core families; 0 for
 * the HBM-bound ones, whose bytes follow from the shapes the caller knows) */
int ee_prof_read_work(int kernel_id, double *work);
int ee_prof_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* EEADV_H */
