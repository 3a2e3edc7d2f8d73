"""Every path that produces BatchNorm batch statistics (ee_bn.hip, ee_fuse.hpp's train_bn_merge, the statistics epilogues of ee_wino.hip /
ee_s2.hip / ee_conv.hip) on the hard channels of tests/bn_reference.py, against its float64 bar - train mode, and eval mode where the path
has one.  The rest of the suite feeds these kernels x = randn * 2 + 0.5 with gamma > 0 and compares with fp32 torch or a sibling kernel.
That includes the sync family, ee_syncbn_{stats,apply,bwd_sums,bwd_apply}_f32 (bn_moments_kernel, bn_sums_kernel, bn_sync_apply_kernel,
bn_sync_bwd_apply_kernel): SyncBatchNorm's local halves, run here for W simulated ranks in this one process - the batch dealt to the ranks
by bn_reference.SYNC_DEALS (ranks of unequal size, of one image, with different slice counts, slices that cut through images, H * W == 4,
70 channels), the all_gather a stack and the all_reduce a sum in rank order - against bn_ref64 over the WHOLE batch.

What is asserted, PER CHANNEL (no allowed error is scaled by a maximum taken over channels):
  * `const` channels (x == 0.75) and the convolution producers' zero-filter channels, train mode: save_mean == the constant,
    save_invstd == fp32 1 / sqrtf(eps), the running statistics moved by exactly momentum * (mean, 0), y == relu(beta [+ residual]) bit for
    bit, dx == 0 where the masked gradient is constant over the channel (bn_reference.hard_case makes the incoming gradient constant
    there; with a residual or a pool in between dz is not constant and dx goes to the float64 bar instead), nothing NaN / inf.
  * every other channel: save_mean, save_invstd, running statistics, y, dx, dresidual, dgamma, dbeta within
        max(4 x the error of torch's stock fp32 F.batch_norm / autograd on the same input and channel, the existing tolerance of the path)
    of bn_ref64, element by element.  The stock error is measured in the same test run; 4 covers another, equally legitimate, fp32
    summation order.  The floors are test_bn_act_matches_torch's: y rtol 1e-5 atol 2e-5; running statistics rtol 1e-5 atol 1e-6 (taken
    for save_mean / save_invstd too: the running statistics are their images under x -> 0.9 r + 0.1 x, so this is the stricter reading);
    dx / dresidual rtol 2e-5 atol 2e-5; dgamma / dbeta rtol 2e-5 atol 2e-5 sqrt(n).  The convolution behind ee_wino3x3_bn_train_pre_f32
    keeps test_gpu_trainfuse.py's 2e-5, of the result channel's own largest entry.
  * masks: outside |pre-activation| <= 1e-4 (under 0.1 % of any case: test_bn_reference_host.py) the fp32 y > 0 equals the float64 one,
    negative gamma included; a gamma == 0 channel follows beta > 0 as a whole; the mask-from-x backward forms (y = NULL) return the bits
    of the mask-from-y forms.
  * two calls give the same bits.
  * the sync family, on top of all of the above for the whole batch put back together: every rank's moments of a `const` channel are
    exactly (0.75, 0, its count); save_mean, save_invstd and both running statistics are the same bits on every rank; each rank's own
    (sum dz, sum dz * xhat) is held to that rank's float64 share (bn_reference.rank_param_grads64) within max(4 x the error of torch's
    stock fp32 autograd with the incoming gradient zeroed outside the rank's images, the dgamma / dbeta floor with n the RANK's element
    count), and their device sum to bn_ref64's dgamma / dbeta; the y = NULL backward, dy given as two addends (dy2) and dresidual asked for
    or left out return the bits of the plain form; the ranks in the opposite order stay inside the same bounds (other bits are allowed).
    eeadv.syncbn's module runs the two-slices case as one rank with the global count taken either way (_EQUAL_SHARDS), and sends an
    input or residual that starts off a 16-byte boundary to nn.SyncBatchNorm's own forward (held to the y and dx floors alone).
The exactness claims on `const` channels are train-mode claims (batch mean 0.75, M2 0).  In eval mode the running statistics stand in, a
`const` channel is an ordinary one and goes to the float64 bar; the gamma == 0 channels stay exact in both modes (y == relu(beta), dx == 0;
their dresidual, dgamma and dbeta go to the bar).
The backward bar holds the ReLU (and the pool's argmax) branch fixed to the fp32 kernel's own, as tests/branch_replay.py does.

Dispatch branches not reachable through eeadv.ops: the non-split vector kernel <1024,4> (workspace == NULL; ops always passes one) is
called through eeadv._native, as are all ee_bn_act_* cases here so that one helper serves them.  The 16-byte-alignment fallback IS
reachable through the wrapper (it accepts a contiguous view that starts one float into its storage).

A note on the channel count the cases use (C = 6, kinds in a cycle of five, gamma in a cycle of six): the `offset` and `outlier`
channels of the bn_act, bn_sum_act and bn_relu_pool cases carry gamma == 0, so their y and dx fall under the exact checks and their
statistics, dgamma and dbeta under the float64 bar; bn_dual's side b (cycle rolled by 2) puts gamma = -1.25 on `offset`.

Stock fp32 errors and the bounds they give, measured on an MI355X (every run prints them with -s, one `BNHARD case | quantity | kind |
kernel error | stock error | bound` line each).  Per case and quantity, for every channel kind: the largest absolute error of torch's fp32
F.batch_norm / autograd against bn_ref64, the largest bound max(4 x that, floor) any element of such a channel is allowed, and the largest
error of the kernel under test - three numbers per kind, in that order.  Train and eval mode, with and without a residual, and the _xa pair
of the pool are folded into one row by their maxima; channels under an exact check are left out of the quantity they are exact in.
dresidual is left out: the stock error is 0 everywhere (it is dy under the fixed mask), so its bound is the floor.  Reading: the bounds of
mean, invstd and the running statistics are the floors nearly everywhere (4 x stock is smaller) - 1e-5 of the value, i.e. of a variance
whose cross term carries over half of it on `outlier`; torch's own dgamma on `offset` and its dx / dgamma behind 1 / sqrt(eps) on `const`
are poor (up to 0.6), so those bounds are loose and the kernels sit two to five orders below them.
bn_act cached<256,2>
  mean            offset 6.7e-08 3.2e-04 6.7e-08  outlier 6.5e-08 8.2e-05 6.5e-08  tail 2.9e-08 1.7e-05 2.9e-08  plain 3.5e-10 4.0e-06 3.5e-10
  invstd          offset 1.6e-06 4.2e-05 1.4e-07  outlier 6.6e-09 2.2e-06 8.6e-10  tail 1.9e-08 7.2e-06 4.1e-08  plain 2.1e-08 5.8e-06 9.1e-09
  running_mean    offset 1.0e-07 3.3e-05 1.0e-07  outlier 1.7e-08 1.0e-05 1.7e-08  tail 1.7e-08 3.7e-06 1.7e-08  plain 7.8e-10 1.3e-06 7.8e-10
  running_var     offset 4.6e-06 1.8e-05 5.2e-08  outlier 6.2e-07 8.3e-05 3.3e-07  tail 7.1e-08 1.5e-05 4.8e-08  plain 2.7e-08 9.8e-06 2.7e-08
  y               const 2.2e-07 6.4e-05 1.4e-07  tail 2.0e-07 5.8e-05 1.9e-07  plain 3.4e-07 6.4e-05 3.4e-07
  dx              const 1.5e-05 2.7e-03 5.9e-06  tail 1.3e-07 5.5e-05 1.8e-07  plain 1.4e-07 5.5e-05 1.4e-07
  dgamma          const 1.2e-05 4.2e-03 1.2e-05  offset 4.4e-03 1.8e-02 4.3e-05  outlier 9.2e-06 4.5e-03 6.0e-06  tail 2.4e-06 9.8e-04 3.3e-06  plain 3.3e-06 8.6e-04 2.6e-06
  dbeta           const 0.0e+00 5.6e-03 0.0e+00  offset 3.6e-06 5.6e-04 2.4e-06  outlier 1.5e-06 5.4e-04 7.3e-08  tail 1.2e-06 7.1e-04 1.5e-06  plain 2.4e-06 6.4e-04 2.4e-06
bn_act cached<256,7>
  mean            offset 9.4e-06 3.2e-04 2.0e-06  outlier 2.2e-07 1.5e-05 2.2e-07  tail 1.3e-07 3.8e-06 2.3e-08  plain 1.1e-07 5.6e-06 1.0e-08
  invstd          offset 5.0e-06 4.1e-05 2.0e-07  outlier 9.1e-09 3.1e-06 5.8e-09  tail 9.5e-08 9.0e-06 2.4e-08  plain 6.1e-08 6.0e-06 9.1e-10
  running_mean    offset 2.8e-07 3.3e-05 2.0e-07  outlier 4.1e-09 3.5e-06 2.6e-08  tail 4.6e-10 2.4e-06 4.6e-10  plain 2.0e-09 1.5e-06 1.7e-09
  running_var     offset 1.2e-06 7.8e-06 6.9e-08  outlier 9.2e-08 3.2e-05 9.2e-08  tail 1.0e-08 1.4e-05 1.0e-08  plain 4.1e-08 9.4e-06 4.1e-08
  y               const 3.4e-07 6.7e-05 1.4e-07  tail 2.6e-07 6.1e-05 2.7e-07  plain 4.7e-07 7.4e-05 4.7e-07
  dx              const 7.7e-06 2.6e-03 9.9e-06  tail 2.9e-07 6.4e-05 2.3e-07  plain 2.4e-07 7.7e-05 2.4e-07
  dgamma          const 4.3e-05 2.3e-02 1.8e-05  offset 4.3e-03 9.8e-02 1.1e-03  outlier 1.1e-05 3.8e-03 4.1e-06  tail 4.7e-06 1.4e-03 9.6e-06  plain 6.7e-06 1.8e-03 5.3e-06
  dbeta           const 0.0e+00 3.2e-02 0.0e+00  offset 5.2e-06 3.7e-03 5.2e-06  outlier 3.2e-06 1.6e-03 3.2e-06  tail 4.9e-06 1.7e-03 4.9e-06  plain 4.6e-06 1.7e-03 2.8e-06
bn_act cached<1024,7>
  mean            offset 5.3e-06 3.2e-04 3.4e-06  outlier 6.9e-08 5.1e-06 9.1e-09  tail 5.4e-09 1.9e-06 5.4e-09  plain 1.2e-07 6.1e-06 2.2e-09
  invstd          offset 1.5e-06 4.1e-05 4.3e-08  outlier 1.2e-08 4.6e-06 1.2e-08  tail 2.8e-08 1.0e-05 2.8e-08  plain 2.0e-08 6.1e-06 3.9e-08
  running_mean    offset 1.4e-07 3.3e-05 3.4e-07  outlier 1.1e-08 2.5e-06 3.5e-09  tail 4.6e-09 2.2e-06 4.6e-09  plain 7.2e-09 1.5e-06 2.4e-10
  running_var     offset 4.9e-06 1.9e-05 4.4e-08  outlier 5.3e-08 1.8e-05 6.6e-08  tail 9.4e-08 1.3e-05 2.5e-08  plain 6.0e-09 9.4e-06 6.6e-08
  y               const 3.4e-07 6.4e-05 1.4e-07  tail 3.6e-07 6.5e-05 3.1e-07  plain 3.9e-07 7.4e-05 3.9e-07
  dx              const 7.8e-06 2.5e-03 8.2e-06  tail 2.2e-07 6.8e-05 1.9e-07  plain 2.1e-07 7.0e-05 2.1e-07
  dgamma          const 2.4e-04 7.6e-02 4.9e-04  offset 5.7e-02 2.3e-01 7.4e-04  outlier 2.8e-05 3.3e-03 3.2e-05  tail 7.4e-06 3.3e-03 1.5e-05  plain 3.8e-05 5.6e-03 2.3e-05
  dbeta           const 0.0e+00 1.0e-01 0.0e+00  offset 2.7e-05 2.2e-03 7.3e-06  outlier 7.1e-06 2.4e-03 7.1e-06  tail 1.1e-05 3.1e-03 1.2e-05  plain 6.4e-06 3.1e-03 6.4e-06
bn_act cached<1024,7>-edge
  mean            offset 1.2e-05 3.2e-04 7.5e-07  outlier 2.2e-07 6.8e-06 1.3e-07  tail 7.6e-08 2.2e-06 5.9e-09  plain 2.4e-07 6.0e-06 3.3e-08
  invstd          offset 6.2e-07 4.1e-05 1.4e-07  outlier 1.1e-08 4.1e-06 1.1e-08  tail 4.6e-08 9.9e-06 7.3e-08  plain 3.4e-08 6.0e-06 2.6e-08
  running_mean    offset 1.2e-07 3.3e-05 1.2e-07  outlier 9.5e-10 2.7e-06 1.4e-08  tail 4.3e-09 2.2e-06 4.3e-09  plain 7.8e-09 1.5e-06 4.0e-09
  running_var     offset 2.4e-06 9.7e-06 7.5e-08  outlier 1.8e-07 2.0e-05 5.8e-08  tail 2.9e-08 1.3e-05 2.9e-08  plain 2.3e-08 9.4e-06 3.7e-08
  y               const 3.4e-07 7.3e-05 1.4e-07  tail 4.1e-07 6.8e-05 4.3e-07  plain 5.5e-07 8.6e-05 5.5e-07
  dx              const 4.2e-06 2.6e-03 6.4e-06  tail 2.4e-07 7.7e-05 3.8e-07  plain 2.3e-07 7.8e-05 2.3e-07
  dgamma          const 2.7e-01 1.1e+00 6.2e-04  offset 3.0e-02 1.2e-01 1.3e-03  outlier 1.5e-05 3.7e-03 7.8e-06  tail 2.6e-05 7.5e-03 4.8e-05  plain 3.1e-05 1.4e-02 4.8e-05
  dbeta           const 0.0e+00 2.9e-01 0.0e+00  offset 5.2e-05 6.5e-03 5.5e-05  outlier 1.4e-06 3.9e-03 2.1e-05  tail 2.3e-05 8.3e-03 1.8e-05  plain 3.6e-05 7.4e-03 3.5e-05
bn_act split-4-slices
  mean            offset 2.3e-06 3.2e-04 3.9e-07  outlier 1.1e-07 5.8e-06 1.0e-08  tail 1.3e-08 2.0e-06 9.3e-09  plain 3.8e-08 6.0e-06 8.4e-09
  invstd          offset 3.5e-08 4.1e-05 2.7e-07  outlier 2.5e-08 4.3e-06 2.5e-08  tail 5.4e-08 1.0e-05 5.4e-08  plain 9.0e-09 6.0e-06 9.0e-09
  running_mean    offset 1.5e-07 3.3e-05 8.7e-08  outlier 1.4e-09 2.6e-06 1.4e-09  tail 1.5e-10 2.2e-06 7.6e-09  plain 2.1e-09 1.5e-06 1.6e-09
  running_var     offset 6.2e-06 2.5e-05 2.4e-08  outlier 1.1e-07 1.9e-05 1.1e-07  tail 3.3e-09 1.3e-05 3.3e-09  plain 5.6e-08 9.5e-06 5.6e-08
  y               const 3.4e-07 7.2e-05 1.4e-07  tail 3.1e-07 6.3e-05 3.2e-07  plain 4.9e-07 8.7e-05 4.9e-07
  dx              const 5.7e-01 2.3e+00 7.3e-06  tail 2.6e-07 7.8e-05 4.0e-07  plain 2.3e-07 7.3e-05 2.3e-07
  dgamma          const 2.8e-01 1.1e+00 7.4e-04  offset 8.6e-02 3.4e-01 7.8e-04  outlier 3.6e-05 5.4e-03 3.6e-05  tail 2.5e-05 7.7e-03 4.1e-05  plain 2.5e-05 4.8e-03 2.0e-05
  dbeta           const 0.0e+00 3.0e-01 0.0e+00  offset 6.4e-05 9.0e-03 2.8e-05  outlier 2.5e-05 3.8e-03 6.8e-07  tail 1.8e-05 6.8e-03 4.0e-05  plain 1.3e-05 4.5e-03 1.2e-05
bn_act scalar<256,1>
  mean            offset 1.6e-07 3.2e-04 1.6e-07  outlier 1.3e-06 5.5e-05 1.1e-07  tail 4.7e-08 9.5e-06 4.7e-08  plain 4.8e-08 7.7e-06 4.8e-08
  invstd          offset 3.7e-06 4.2e-05 3.1e-07  outlier 1.4e-08 2.3e-06 8.1e-09  tail 5.6e-08 6.7e-06 5.6e-08  plain 2.6e-09 6.1e-06 2.6e-09
  running_mean    offset 3.1e-08 3.3e-05 3.1e-08  outlier 4.5e-09 7.5e-06 4.5e-09  tail 2.3e-09 3.0e-06 2.3e-09  plain 8.3e-09 1.7e-06 8.3e-09
  running_var     offset 3.4e-06 1.3e-05 7.1e-08  outlier 3.0e-07 7.5e-05 3.0e-07  tail 2.2e-08 1.5e-05 9.8e-08  plain 6.4e-08 9.3e-06 4.8e-09
  y               const 2.2e-07 6.4e-05 1.4e-07  tail 1.7e-07 4.5e-05 2.3e-07  plain 2.2e-07 5.4e-05 2.2e-07
  dx              const 7.1e-06 2.7e-03 1.1e-05  tail 1.1e-07 5.3e-05 1.5e-07  plain 7.8e-08 4.6e-05 6.7e-08
  dgamma          const 3.0e-07 9.6e-04 3.0e-07  offset 8.1e-04 7.2e-03 6.8e-05  outlier 1.4e-06 4.9e-04 1.4e-06  tail 4.2e-07 2.9e-04 6.5e-07  plain 2.7e-07 3.2e-04 1.6e-06
  dbeta           const 0.0e+00 1.3e-03 0.0e+00  offset 1.0e-06 3.9e-04 6.6e-07  outlier 4.2e-07 2.9e-04 4.2e-07  tail 3.6e-07 3.3e-04 9.3e-07  plain 2.2e-07 2.6e-04 2.2e-07
bn_act scalar<1024,1>
  mean            offset 3.6e-06 3.2e-04 1.9e-07  outlier 1.7e-08 3.2e-06 1.3e-08  tail 2.1e-10 1.5e-06 2.1e-10  plain 4.8e-08 6.0e-06 1.1e-08
  invstd          offset 9.1e-07 4.1e-05 4.2e-08  outlier 6.8e-08 5.6e-06 2.1e-08  tail 2.0e-08 1.0e-05 2.0e-08  plain 3.2e-08 6.0e-06 2.8e-08
  running_mean    offset 1.9e-08 3.3e-05 1.9e-08  outlier 9.1e-11 2.3e-06 9.1e-11  tail 1.2e-09 2.2e-06 6.2e-09  plain 4.0e-10 1.5e-06 4.0e-10
  running_var     offset 6.7e-06 2.7e-05 6.2e-08  outlier 1.1e-07 1.5e-05 1.2e-08  tail 1.7e-08 1.3e-05 1.7e-08  plain 1.6e-08 9.4e-06 4.4e-08
  y               const 3.4e-07 7.1e-05 1.4e-07  tail 4.3e-07 7.2e-05 2.9e-07  plain 6.0e-07 8.5e-05 6.0e-07
  dx              const 7.1e-06 2.6e-03 9.4e-06  tail 6.2e-07 8.3e-05 2.5e-07  plain 2.1e-07 7.7e-05 2.1e-07
  dgamma          const 3.6e-04 1.3e-01 1.8e-03  offset 1.3e-01 5.3e-01 1.1e-03  outlier 3.0e-06 3.5e-03 6.5e-06  tail 1.3e-05 4.1e-03 1.4e-05  plain 2.0e-05 4.7e-03 5.6e-05
  dbeta           const 0.0e+00 1.8e-01 0.0e+00  offset 2.3e-05 3.4e-03 1.2e-05  outlier 2.5e-06 3.8e-03 9.0e-06  tail 2.0e-05 4.6e-03 1.2e-05  plain 1.2e-05 6.9e-03 4.9e-05
bn_act vector<1024,4>-no-workspace
  mean            offset 2.3e-06 3.2e-04 3.9e-07  outlier 1.1e-07 5.8e-06 1.0e-08  tail 1.3e-08 2.0e-06 1.3e-08  plain 3.8e-08 6.0e-06 8.4e-09
  invstd          offset 3.5e-08 4.1e-05 2.7e-07  outlier 2.5e-08 4.3e-06 4.4e-09  tail 5.4e-08 1.0e-05 5.5e-09  plain 9.0e-09 6.0e-06 9.0e-09
  running_mean    offset 1.5e-07 3.3e-05 8.7e-08  outlier 1.4e-09 2.6e-06 1.4e-09  tail 1.5e-10 2.2e-06 1.5e-10  plain 2.1e-09 1.5e-06 1.6e-09
  running_var     offset 6.2e-06 2.5e-05 2.4e-08  outlier 1.1e-07 1.9e-05 6.6e-09  tail 3.3e-09 1.3e-05 3.3e-09  plain 5.6e-08 9.5e-06 5.6e-08
  y               const 3.4e-07 7.2e-05 1.4e-07  tail 3.1e-07 6.3e-05 3.0e-07  plain 4.9e-07 8.7e-05 4.9e-07
  dx              const 5.7e-01 2.3e+00 7.3e-06  tail 2.6e-07 7.8e-05 2.0e-07  plain 2.3e-07 7.3e-05 2.3e-07
  dgamma          const 2.8e-01 1.1e+00 7.4e-04  offset 8.6e-02 3.4e-01 2.2e-03  outlier 3.6e-05 5.4e-03 2.9e-05  tail 2.5e-05 7.7e-03 2.9e-05  plain 2.5e-05 4.8e-03 5.6e-05
  dbeta           const 0.0e+00 3.0e-01 0.0e+00  offset 6.4e-05 9.0e-03 2.8e-05  outlier 2.5e-05 3.8e-03 1.6e-05  tail 1.8e-05 6.8e-03 1.8e-05  plain 1.3e-05 4.5e-03 2.2e-05
bn_act alignment-fallback
  mean            offset 9.4e-06 3.2e-04 3.7e-06  outlier 2.2e-07 1.5e-05 9.7e-08  tail 1.3e-07 3.8e-06 2.3e-08  plain 1.1e-07 5.6e-06 1.9e-08
  invstd          offset 5.0e-06 4.1e-05 2.0e-07  outlier 9.1e-09 3.1e-06 5.8e-09  tail 9.5e-08 9.0e-06 2.4e-08  plain 6.1e-08 6.0e-06 9.1e-10
  running_mean    offset 2.8e-07 3.3e-05 2.8e-07  outlier 4.1e-09 3.5e-06 4.1e-09  tail 4.6e-10 2.4e-06 4.6e-10  plain 2.0e-09 1.5e-06 2.0e-09
  running_var     offset 1.2e-06 7.8e-06 6.9e-08  outlier 9.2e-08 3.2e-05 9.2e-08  tail 1.0e-08 1.4e-05 1.0e-08  plain 4.1e-08 9.4e-06 4.1e-08
  y               const 3.4e-07 6.7e-05 1.4e-07  tail 2.6e-07 6.1e-05 2.7e-07  plain 4.7e-07 7.4e-05 4.7e-07
  dx              const 7.7e-06 2.6e-03 9.9e-06  tail 2.9e-07 6.4e-05 2.3e-07  plain 2.4e-07 7.7e-05 2.4e-07
  dgamma          const 4.3e-05 2.3e-02 4.3e-05  offset 4.3e-03 9.8e-02 2.0e-03  outlier 1.1e-05 3.8e-03 1.1e-05  tail 4.7e-06 1.4e-03 4.9e-06  plain 6.7e-06 1.8e-03 1.3e-05
  dbeta           const 0.0e+00 3.2e-02 0.0e+00  offset 5.2e-06 3.7e-03 5.2e-06  outlier 3.2e-06 1.6e-03 6.0e-07  tail 4.9e-06 1.7e-03 6.3e-06  plain 4.6e-06 1.7e-03 7.8e-06
bn_dual side a
  mean            offset 1.9e-06 3.2e-04 1.9e-06  outlier 6.1e-08 2.0e-05 1.8e-07  tail 8.3e-09 4.2e-06 8.3e-09  plain 6.2e-10 6.0e-06 5.9e-08
  invstd          offset 5.3e-07 4.3e-05 5.4e-08  outlier 3.2e-09 2.8e-06 1.2e-08  tail 3.8e-08 8.6e-06 8.2e-08  plain 1.0e-08 6.0e-06 1.0e-08
  running_mean    offset 1.9e-07 3.3e-05 2.9e-07  outlier 2.0e-08 4.0e-06 2.0e-08  tail 1.9e-09 2.4e-06 1.9e-09  plain 4.4e-09 1.5e-06 4.4e-09
  running_var     offset 4.2e-06 1.7e-05 5.7e-08  outlier 5.8e-08 4.0e-05 5.8e-08  tail 2.9e-08 1.4e-05 2.9e-08  plain 5.1e-09 9.5e-06 5.1e-09
  y               const 1.3e-07 3.6e-05 7.4e-09  offset 2.0e-07 4.7e-05 1.6e-07  outlier 1.3e-07 3.9e-05 1.1e-07  tail 2.7e-07 4.8e-05 2.3e-07  plain 4.9e-04 1.9e-03 7.7e-07
  dx              const 3.6e-08 3.7e-05 3.6e-08  offset 0.0e+00 2.0e-05 0.0e+00  outlier 0.0e+00 2.0e-05 0.0e+00  tail 2.4e-07 7.3e-05 2.8e-07  plain 6.4e-08 3.2e-05 3.6e-08
  dgamma          const 7.6e-06 2.4e-03 1.1e-08  offset 2.1e-04 2.9e-03 9.9e-05  outlier 2.1e-06 8.7e-04 5.5e-06  tail 1.5e-06 5.8e-04 8.7e-07  plain 7.4e-07 5.4e-04 1.7e-06
  dbeta           const 0.0e+00 3.2e-03 0.0e+00  offset 7.6e-07 5.8e-04 7.1e-07  outlier 3.5e-07 4.3e-04 8.3e-07  tail 1.3e-06 6.4e-04 1.4e-06  plain 3.3e-07 3.9e-04 3.3e-07
bn_dual side b
  mean            offset 8.6e-08 3.2e-04 8.6e-08  outlier 9.8e-08 1.9e-05 7.6e-08  tail 1.4e-08 4.2e-06 1.6e-08  plain 4.7e-08 8.2e-06 1.3e-08
  invstd          offset 1.2e-06 4.1e-05 1.5e-08  outlier 1.3e-08 3.0e-06 1.3e-08  tail 5.3e-08 8.6e-06 6.8e-09  plain 2.8e-08 5.9e-06 2.8e-08
  running_mean    offset 8.7e-08 3.3e-05 8.7e-08  outlier 1.0e-08 3.8e-06 1.7e-08  tail 2.4e-09 1.3e-06 1.3e-09  plain 5.2e-09 2.8e-06 5.2e-09
  running_var     offset 2.0e-06 8.1e-06 2.4e-08  outlier 1.3e-07 3.2e-05 1.1e-07  tail 9.0e-09 9.5e-06 9.0e-09  plain 3.0e-08 1.4e-05 3.0e-08
  dx              const 1.8e-04 3.7e-02 9.2e-05  offset 1.9e-03 7.4e-03 1.1e-06  outlier 0.0e+00 2.0e-05 0.0e+00  tail 2.0e-07 7.9e-05 1.3e-07  plain 5.8e-08 4.7e-05 5.8e-08
  dgamma          const 1.7e-07 4.9e-04 1.7e-07  offset 2.5e-04 9.9e-04 1.4e-06  outlier 2.8e-06 5.6e-03 2.8e-05  tail 3.6e-06 4.0e-04 3.1e-06  plain 9.2e-07 7.1e-04 9.2e-07
  dbeta           const 1.3e-06 6.4e-04 1.4e-06  offset 3.3e-07 3.9e-04 3.3e-07  outlier 0.0e+00 3.2e-03 0.0e+00  tail 7.6e-07 5.8e-04 7.1e-07  plain 3.5e-07 4.3e-04 8.3e-07
bn_sum_act cached<256,2>
  mean            offset 2.1e-07 3.2e-04 2.1e-07  outlier 2.4e-07 8.3e-05 2.4e-07  tail 3.8e-08 1.6e-05 3.8e-08  plain 3.7e-08 7.1e-06 3.7e-08
  invstd          offset 1.2e-06 4.0e-05 2.5e-07  outlier 6.3e-09 2.2e-06 8.6e-09  tail 3.6e-08 6.9e-06 2.3e-08  plain 1.7e-08 6.0e-06 1.7e-08
  running_mean    offset 7.4e-08 3.3e-05 7.4e-08  outlier 4.8e-08 1.0e-05 4.8e-08  tail 7.7e-09 3.6e-06 7.7e-09  plain 3.9e-09 1.6e-06 3.6e-09
  running_var     offset 6.5e-06 2.6e-05 4.9e-08  outlier 4.4e-07 8.4e-05 4.4e-07  tail 8.4e-08 1.5e-05 3.5e-08  plain 1.2e-08 9.5e-06 1.2e-08
  y               const 9.7e-08 3.2e-05 2.2e-08  tail 2.1e-07 4.1e-05 2.1e-07  plain 2.2e-07 6.0e-05 2.2e-07
  dx              const 3.6e-08 3.7e-05 3.6e-08  tail 1.4e-07 5.3e-05 1.4e-07  plain 1.7e-07 6.6e-05 1.7e-07
  dgamma          const 2.0e-08 4.2e-03 2.0e-08  offset 8.4e-03 3.4e-02 4.2e-05  outlier 0.0e+00 4.5e-04 0.0e+00  tail 3.9e-07 5.7e-04 5.7e-07  plain 1.5e-06 5.7e-04 1.8e-06
  dbeta           const 0.0e+00 5.6e-03 0.0e+00  offset 6.0e-07 5.7e-04 8.3e-07  outlier 0.0e+00 4.5e-04 0.0e+00  tail 1.4e-06 4.8e-04 9.5e-07  plain 1.8e-06 5.6e-04 1.2e-06
bn_sum_act cached<256,7>
  mean            offset 6.7e-06 3.2e-04 9.4e-07  outlier 3.9e-07 1.5e-05 1.5e-07  tail 6.5e-08 3.5e-06 5.8e-09  plain 9.6e-08 5.7e-06 6.6e-09
  invstd          offset 3.5e-06 4.1e-05 1.2e-07  outlier 3.7e-08 3.1e-06 8.2e-09  tail 3.9e-08 8.9e-06 2.0e-08  plain 7.0e-09 6.0e-06 2.3e-08
  running_mean    offset 7.2e-07 3.3e-05 1.6e-09  outlier 4.7e-09 3.5e-06 2.5e-08  tail 3.9e-10 2.4e-06 3.9e-10  plain 3.9e-11 1.5e-06 3.9e-11
  running_var     offset 4.3e-05 1.7e-04 5.3e-08  outlier 1.2e-07 3.3e-05 1.2e-07  tail 3.3e-08 1.4e-05 3.3e-08  plain 5.8e-08 9.5e-06 6.1e-08
  y               const 9.7e-08 3.2e-05 2.2e-08  tail 2.4e-07 4.2e-05 1.5e-07  plain 2.8e-07 5.9e-05 2.8e-07
  dx              const 3.6e-08 3.7e-05 3.6e-08  tail 1.7e-07 5.8e-05 2.0e-07  plain 1.4e-07 7.0e-05 1.4e-07
  dgamma          const 1.2e-07 2.3e-02 1.2e-07  offset 3.7e-02 1.5e-01 3.4e-04  outlier 0.0e+00 1.1e-03 0.0e+00  tail 6.7e-06 1.7e-03 6.7e-06  plain 7.3e-06 1.4e-03 4.1e-06
  dbeta           const 0.0e+00 3.2e-02 0.0e+00  offset 4.3e-07 1.6e-03 3.4e-06  outlier 0.0e+00 1.1e-03 0.0e+00  tail 2.0e-06 1.4e-03 4.2e-06  plain 1.3e-06 1.3e-03 1.6e-06
bn_sum_act cached<1024,7>
  mean            offset 5.9e-06 3.2e-04 1.8e-06  outlier 5.1e-08 5.1e-06 3.8e-08  tail 1.8e-08 1.8e-06 4.6e-09  plain 7.0e-08 6.2e-06 1.0e-08
  invstd          offset 1.0e-06 4.1e-05 5.0e-08  outlier 3.0e-08 4.6e-06 4.7e-10  tail 1.3e-08 1.0e-05 1.3e-08  plain 7.8e-09 6.0e-06 2.2e-08
  running_mean    offset 2.5e-07 3.3e-05 2.2e-07  outlier 1.3e-08 2.5e-06 1.7e-09  tail 3.5e-10 2.2e-06 3.5e-10  plain 9.7e-10 1.5e-06 9.7e-10
  running_var     offset 2.0e-05 7.9e-05 2.0e-08  outlier 5.3e-08 1.8e-05 1.7e-07  tail 2.0e-08 1.3e-05 2.0e-08  plain 2.5e-10 9.5e-06 2.5e-10
  y               const 9.7e-08 3.2e-05 2.2e-08  tail 2.8e-07 4.8e-05 2.8e-07  plain 3.4e-07 7.8e-05 3.4e-07
  dx              const 3.6e-08 3.7e-05 3.6e-08  tail 2.6e-07 7.3e-05 1.4e-07  plain 2.0e-07 7.3e-05 2.0e-07
  dgamma          const 2.4e-04 7.6e-02 4.9e-04  offset 5.2e-02 2.1e-01 1.4e-03  outlier 0.0e+00 2.0e-03 0.0e+00  tail 5.7e-06 2.3e-03 1.4e-05  plain 1.6e-05 5.1e-03 1.8e-05
  dbeta           const 0.0e+00 1.0e-01 0.0e+00  offset 8.6e-06 6.0e-03 6.6e-06  outlier 0.0e+00 2.0e-03 0.0e+00  tail 3.1e-06 3.3e-03 3.1e-06  plain 6.0e-06 2.6e-03 4.1e-06
bn_relu_pool one-group
  mean            offset 3.1e-06 3.2e-04 7.5e-07  outlier 2.1e-07 5.4e-05 2.6e-07  tail 6.1e-08 1.1e-05 1.7e-09  plain 4.5e-08 5.6e-06 1.5e-08
  invstd          offset 7.2e-07 4.1e-05 2.4e-07  outlier 9.5e-09 2.3e-06 5.4e-09  tail 3.8e-08 7.0e-06 3.8e-08  plain 4.5e-08 6.1e-06 1.5e-08
  running_mean    offset 3.1e-07 3.3e-05 1.7e-07  outlier 6.7e-09 7.5e-06 6.6e-08  tail 1.1e-09 3.1e-06 1.1e-09  plain 1.6e-09 1.5e-06 1.6e-09
  running_var     offset 1.5e-05 6.0e-05 2.0e-08  outlier 4.6e-08 7.1e-05 4.3e-07  tail 5.2e-09 1.5e-05 5.2e-09  plain 3.5e-08 9.4e-06 3.5e-08
  yp              const 9.7e-08 3.2e-05 2.2e-08  tail 1.6e-07 4.4e-05 2.0e-07  plain 2.0e-07 6.2e-05 2.0e-07
  dx              const 1.7e-05 3.6e-03 1.4e-05  offset 0.0e+00 2.0e-05 0.0e+00  outlier 0.0e+00 2.0e-05 0.0e+00  tail 9.3e-08 5.4e-05 8.3e-08  plain 1.8e-07 6.8e-05 1.8e-07
  dgamma          const 1.9e-06 8.6e-04 2.8e-09  offset 1.2e-02 4.7e-02 4.1e-05  outlier 0.0e+00 3.4e-04 0.0e+00  tail 1.5e-06 4.8e-04 1.1e-06  plain 3.6e-06 1.8e-03 4.0e-06
  dbeta           const 0.0e+00 1.1e-03 0.0e+00  offset 7.7e-08 6.1e-04 7.7e-08  outlier 0.0e+00 3.4e-04 0.0e+00  tail 4.0e-07 4.9e-04 4.0e-07  plain 1.1e-06 6.7e-04 1.1e-06
bn_relu_pool two-images-per-group
  mean            offset 2.2e-06 3.2e-04 1.6e-06  outlier 8.3e-08 3.7e-06 6.6e-09  tail 9.6e-09 1.1e-06 3.3e-10  plain 1.4e-07 6.2e-06 2.3e-08
  invstd          offset 1.6e-06 4.1e-05 1.9e-07  outlier 2.4e-08 5.4e-06 5.9e-09  tail 3.6e-08 1.0e-05 3.6e-08  plain 1.3e-08 6.1e-06 1.3e-08
  running_mean    offset 2.2e-07 3.3e-05 2.5e-07  outlier 9.8e-09 2.4e-06 9.8e-09  tail 8.6e-10 2.1e-06 8.6e-10  plain 2.3e-09 1.5e-06 2.3e-09
  running_var     offset 1.1e-05 4.6e-05 5.1e-08  outlier 6.3e-08 1.5e-05 6.3e-08  tail 5.7e-09 1.3e-05 5.7e-09  plain 1.0e-09 9.4e-06 1.0e-09
  yp              const 9.7e-08 3.2e-05 2.2e-08  tail 2.5e-07 4.3e-05 1.8e-07  plain 3.6e-07 7.1e-05 3.6e-07
  dx              const 7.8e-06 3.6e-03 1.4e-05  offset 0.0e+00 2.0e-05 0.0e+00  outlier 0.0e+00 2.0e-05 0.0e+00  tail 3.0e-07 8.2e-05 3.7e-07  plain 3.7e-07 9.3e-05 3.7e-07
  dgamma          const 1.9e-06 7.2e-03 1.9e-06  offset 8.7e-03 3.5e-02 2.2e-04  outlier 0.0e+00 1.2e-03 0.0e+00  tail 3.8e-06 2.0e-03 7.6e-06  plain 6.5e-06 2.4e-03 1.2e-05
  dbeta           const 0.0e+00 9.6e-03 0.0e+00  offset 2.8e-06 1.9e-03 6.6e-06  outlier 0.0e+00 1.2e-03 0.0e+00  tail 1.4e-06 1.7e-03 3.3e-06  plain 2.6e-06 1.8e-03 8.3e-06
bn_relu_pool conv_stats
  mean            conv-out 1.9e-06 9.5e-05 5.3e-07
  invstd          conv-out 2.5e-08 3.9e-06 2.9e-08
  running_mean    conv-out 8.5e-08 1.2e-05 6.5e-08
  running_var     conv-out 1.8e-06 1.2e-04 1.0e-06
  yp              conv-out 9.3e-07 9.8e-05 7.5e-07
  dx              zero-filter 9.2e-05 3.2e-02 1.3e-04  conv-out 1.9e-07 5.2e-05 2.1e-07
  dgamma          zero-filter 0.0e+00 4.4e-04 0.0e+00  conv-out 4.4e-06 9.3e-04 4.1e-06
  dbeta           zero-filter 2.5e-06 7.8e-04 2.5e-06  conv-out 1.9e-06 8.2e-04 1.9e-06
wino_stats H=4 C=32
  mean            conv-out 9.3e-07 7.0e-05 8.1e-07
  invstd          conv-out 2.1e-08 4.1e-06 2.6e-08
  running_mean    conv-out 1.1e-07 9.0e-06 7.2e-08
  running_var     conv-out 1.8e-06 8.1e-05 1.1e-06
  conv2(relu(bn)) conv-out 9.0e-07 9.7e-05 7.4e-07
wino_stats H=8 C=32
  mean            conv-out 7.5e-07 6.1e-05 3.8e-07
  invstd          conv-out 2.9e-08 4.2e-06 2.5e-08
  running_mean    conv-out 4.6e-08 7.0e-06 4.6e-08
  running_var     conv-out 6.5e-07 6.9e-05 5.9e-07
  conv2(relu(bn)) conv-out 8.1e-07 1.0e-04 7.6e-07
wino_stats H=16 C=32
  mean            conv-out 6.2e-07 6.6e-05 6.2e-07
  invstd          conv-out 1.9e-08 3.8e-06 2.5e-08
  running_mean    conv-out 8.7e-08 8.2e-06 5.0e-08
  running_var     conv-out 1.3e-06 6.5e-05 9.4e-07
  conv2(relu(bn)) conv-out 1.2e-06 9.7e-05 8.6e-07
wino_bwd_pre H=16
  conv1^T(bn_bwd) conv-out 2.7e-07 2.1e-05 2.6e-07
pair_stats H=8 mt=222111
  mean            conv-out 9.7e-07 1.1e-04 5.2e-07
  invstd          conv-out 3.0e-08 4.4e-06 3.0e-08
  running_mean    conv-out 1.3e-07 1.3e-05 7.3e-08
  running_var     conv-out 1.6e-06 1.6e-04 1.5e-06
  conv2(relu(bn)) conv-out 1.2e-06 9.8e-05 8.8e-07
pair_stats H=8 mt=111222
  mean            conv-out 9.7e-07 1.1e-04 5.2e-07
  invstd          conv-out 3.0e-08 4.4e-06 3.0e-08
  running_mean    conv-out 1.3e-07 1.3e-05 7.3e-08
  running_var     conv-out 1.6e-06 1.6e-04 1.5e-06
  conv2(relu(bn)) conv-out 1.2e-06 9.8e-05 8.8e-07
pair_stats H=16 mt=222111
  mean            conv-out 7.7e-07 1.2e-04 1.2e-06
  invstd          conv-out 2.5e-08 3.9e-06 2.5e-08
  running_mean    conv-out 6.7e-08 1.1e-05 1.0e-07
  running_var     conv-out 1.9e-06 1.9e-04 1.8e-06
  conv2(relu(bn)) conv-out 1.2e-06 9.3e-05 1.0e-06
pair_stats H=16 mt=111222
  mean            conv-out 7.7e-07 1.2e-04 1.2e-06
  invstd          conv-out 2.5e-08 3.9e-06 2.5e-08
  running_mean    conv-out 6.7e-08 1.1e-05 1.0e-07
  running_var     conv-out 1.9e-06 1.9e-04 1.8e-06
  conv2(relu(bn)) conv-out 1.2e-06 9.3e-05 1.0e-06
The syncbn rows fold every deal of a case, with and without a residual and both rank orders, by their maxima; dgamma_r / dbeta_r are the
ranks' own sums against their float64 shares, folded over the ranks as well.  With C = 6 the `offset` and `outlier` channels carry gamma == 0
(exact y and dx); channels-70 puts every gamma on every kind, and shows torch's own y and dx on `offset` to be poor (4.6e-3, 1.8e-2).
syncbn one-slice
  mean            offset 9.2e-07 3.2e-04 9.2e-07  outlier 1.3e-07 2.2e-05 3.5e-07  tail 6.8e-09 3.0e-06 2.3e-08  plain 1.2e-09 4.2e-06 1.2e-09
  invstd          offset 4.3e-07 3.9e-05 1.2e-06  outlier 4.3e-09 2.7e-06 1.1e-08  tail 1.8e-08 8.5e-06 7.8e-08  plain 3.6e-09 6.1e-06 3.6e-09
  running_mean    offset 3.0e-09 3.3e-05 3.0e-09  outlier 1.6e-08 4.2e-06 4.4e-08  tail 5.6e-10 2.3e-06 5.6e-10  plain 1.6e-09 1.3e-06 1.6e-09
  running_var     offset 6.9e-06 2.8e-05 6.4e-08  outlier 5.6e-07 4.6e-05 8.5e-08  tail 2.7e-08 1.4e-05 2.7e-08  plain 3.8e-08 9.4e-06 3.8e-08
  y               tail 1.3e-07 4.3e-05 1.8e-07  plain 1.5e-07 5.4e-05 1.5e-07
  dx              const 1.1e-05 2.4e-03 7.9e-06  tail 1.9e-07 5.6e-05 1.9e-07  plain 2.9e-08 3.1e-05 2.9e-08
  dgamma          const 0.0e+00 2.3e-04 0.0e+00  offset 5.5e-03 2.2e-02 1.7e-05  outlier 2.1e-07 3.1e-04 7.4e-07  tail 1.0e-06 3.6e-04 1.3e-06  plain 6.7e-07 3.3e-04 1.2e-06
  dbeta           const 0.0e+00 1.5e-03 0.0e+00  offset 2.7e-07 3.2e-04 9.3e-07  outlier 6.9e-08 3.2e-04 1.0e-06  tail 7.3e-07 5.5e-04 7.3e-07  plain 3.2e-07 3.5e-04 6.3e-07
  dgamma_r        const 0.0e+00 2.3e-04 0.0e+00  offset 5.5e-03 2.2e-02 2.6e-05  outlier 2.6e-07 3.1e-04 3.8e-07  tail 1.0e-06 3.6e-04 1.0e-06  plain 6.7e-07 3.3e-04 5.8e-07
  dbeta_r         const 0.0e+00 1.5e-03 0.0e+00  offset 6.8e-07 3.2e-04 1.2e-06  outlier 5.8e-07 3.4e-04 4.4e-07  tail 1.3e-06 5.5e-04 1.3e-06  plain 3.4e-07 3.5e-04 5.0e-07
syncbn hw4
  mean            offset 4.7e-06 3.2e-04 9.0e-07  outlier 9.8e-08 1.9e-05 2.1e-08  tail 2.1e-08 5.5e-06 3.8e-08  plain 3.0e-08 5.2e-06 3.0e-08
  invstd          offset 6.8e-06 4.0e-05 2.3e-06  outlier 1.6e-08 2.9e-06 1.6e-09  tail 5.9e-08 8.3e-06 6.6e-10  plain 7.5e-09 5.7e-06 3.7e-08
  running_mean    offset 5.7e-07 3.3e-05 9.0e-08  outlier 7.3e-09 3.9e-06 7.3e-09  tail 4.3e-09 2.6e-06 4.3e-09  plain 2.3e-09 1.4e-06 1.4e-09
  running_var     offset 4.0e-05 1.6e-04 3.7e-08  outlier 1.5e-07 3.7e-05 1.5e-07  tail 7.0e-09 1.4e-05 7.0e-09  plain 1.0e-07 1.0e-05 1.7e-08
  y               tail 1.2e-07 4.6e-05 2.1e-07  plain 1.5e-07 3.7e-05 1.5e-07
  dx              const 1.0e-05 2.7e-03 1.1e-05  tail 7.3e-08 4.2e-05 5.1e-08  plain 4.1e-08 2.9e-05 4.2e-08
  dgamma          const 0.0e+00 1.2e-04 0.0e+00  offset 6.4e-03 2.5e-02 2.1e-05  outlier 8.3e-08 1.5e-04 3.6e-08  tail 8.3e-08 1.7e-04 1.6e-07  plain 1.3e-07 1.5e-04 1.1e-07
  dbeta           const 0.0e+00 4.8e-04 0.0e+00  offset 4.5e-08 2.4e-04 4.5e-08  outlier 4.7e-08 1.5e-04 1.7e-07  tail 1.6e-07 1.9e-04 1.6e-07  plain 2.9e-07 1.5e-04 2.9e-07
  dgamma_r        const 0.0e+00 8.9e-05 0.0e+00  offset 7.7e-03 3.1e-02 8.0e-06  outlier 2.6e-08 1.2e-04 1.1e-07  tail 5.7e-08 1.3e-04 1.9e-07  plain 1.8e-07 1.3e-04 2.9e-07
  dbeta_r         const 0.0e+00 2.9e-04 0.0e+00  offset 1.8e-07 1.4e-04 2.2e-07  outlier 1.3e-07 1.4e-04 1.3e-07  tail 1.4e-07 1.5e-04 1.4e-07  plain 2.6e-07 1.4e-04 2.6e-07
syncbn two-slices
  mean            offset 8.4e-06 3.2e-04 3.1e-06  outlier 7.6e-07 2.4e-05 2.8e-07  tail 6.1e-08 5.2e-06 8.8e-08  plain 1.4e-07 6.1e-06 2.0e-08
  invstd          offset 3.5e-07 4.1e-05 1.3e-07  outlier 5.1e-09 2.7e-06 9.8e-09  tail 1.8e-08 8.1e-06 4.2e-08  plain 5.4e-09 6.0e-06 5.4e-09
  running_mean    offset 3.6e-07 3.3e-05 3.6e-07  outlier 3.7e-08 4.4e-06 3.7e-08  tail 2.7e-09 2.5e-06 1.2e-08  plain 2.7e-09 1.5e-06 2.7e-09
  running_var     offset 4.1e-05 1.6e-04 3.8e-08  outlier 3.2e-08 4.5e-05 4.4e-07  tail 1.1e-08 1.4e-05 1.1e-08  plain 3.7e-08 9.5e-06 3.7e-08
  y               tail 3.7e-07 7.2e-05 3.1e-07  plain 3.0e-07 7.5e-05 3.0e-07
  dx              const 6.8e-06 2.6e-03 9.8e-06  tail 3.3e-07 6.5e-05 3.3e-07  plain 1.3e-07 4.2e-05 9.3e-08
  dgamma          const 0.0e+00 3.0e-03 0.0e+00  offset 4.0e-01 1.6e+00 3.2e-04  outlier 1.2e-05 3.9e-03 7.5e-06  tail 2.1e-05 5.5e-03 1.3e-05  plain 1.2e-05 5.3e-03 2.1e-05
  dbeta           const 0.0e+00 2.2e-01 0.0e+00  offset 7.7e-06 3.5e-03 2.1e-05  outlier 4.8e-06 4.0e-03 8.6e-06  tail 4.9e-06 6.2e-03 2.6e-05  plain 2.2e-05 7.3e-03 2.2e-05
  dgamma_r        const 0.0e+00 2.5e-03 0.0e+00  offset 3.7e-01 1.5e+00 7.8e-04  outlier 8.5e-06 3.6e-03 1.0e-05  tail 2.5e-05 4.7e-03 1.1e-05  plain 1.8e-05 5.3e-03 2.0e-05
  dbeta_r         const 0.0e+00 1.6e-01 0.0e+00  offset 1.6e-05 3.8e-03 1.3e-05  outlier 1.2e-05 3.0e-03 8.0e-06  tail 1.2e-05 5.5e-03 2.1e-05  plain 1.5e-05 5.3e-03 1.2e-05
syncbn four-slices
  mean            offset 6.0e-06 3.2e-04 1.6e-06  outlier 6.2e-08 1.4e-05 1.8e-07  tail 8.1e-09 3.4e-06 2.2e-08  plain 1.4e-08 5.9e-06 1.4e-08
  invstd          offset 3.8e-07 4.1e-05 1.4e-07  outlier 2.4e-09 3.1e-06 2.4e-09  tail 4.9e-09 8.9e-06 4.9e-09  plain 4.2e-09 6.0e-06 3.4e-08
  running_mean    offset 2.7e-07 3.3e-05 2.1e-07  outlier 2.6e-08 3.5e-06 1.9e-08  tail 1.1e-08 2.4e-06 1.1e-08  plain 4.6e-09 1.5e-06 2.9e-09
  running_var     offset 1.2e-05 5.0e-05 5.0e-08  outlier 6.0e-08 3.2e-05 4.2e-07  tail 1.4e-08 1.4e-05 1.4e-08  plain 4.3e-08 9.5e-06 4.3e-08
  y               tail 3.4e-07 6.9e-05 2.6e-07  plain 2.2e-07 6.6e-05 4.1e-07
  dx              const 1.8e-05 2.6e-03 1.3e-05  tail 2.9e-07 7.5e-05 2.3e-07  plain 1.1e-07 4.0e-05 1.3e-07
  dgamma          const 0.0e+00 3.9e-03 0.0e+00  offset 8.8e-02 3.5e-01 3.7e-04  outlier 6.6e-06 4.7e-03 1.6e-05  tail 1.5e-05 5.9e-03 1.8e-05  plain 3.2e-05 7.4e-03 1.7e-05
  dbeta           const 0.0e+00 3.8e-01 0.0e+00  offset 1.5e-05 5.1e-03 4.2e-05  outlier 1.3e-05 4.3e-03 1.8e-05  tail 1.2e-05 6.6e-03 2.3e-05  plain 6.1e-06 9.5e-03 3.7e-05
  dgamma_r        const 0.0e+00 3.4e-03 0.0e+00  offset 1.3e-01 5.0e-01 4.0e-04  outlier 7.7e-06 4.4e-03 1.5e-05  tail 6.9e-06 4.7e-03 1.3e-05  plain 1.4e-05 5.4e-03 2.1e-05
  dbeta_r         const 0.0e+00 2.9e-01 0.0e+00  offset 1.8e-05 4.7e-03 2.9e-05  outlier 8.8e-06 4.6e-03 1.2e-05  tail 1.9e-05 5.5e-03 1.9e-05  plain 8.5e-06 7.6e-03 3.0e-05
syncbn channels-70
  mean            offset 2.9e-06 3.2e-04 2.4e-06  outlier 4.5e-07 4.6e-05 7.0e-07  tail 5.0e-08 1.1e-05 1.6e-07  plain 2.1e-08 1.1e-05 9.9e-08
  invstd          offset 1.1e-05 5.5e-05 6.8e-06  outlier 2.2e-08 2.5e-06 1.5e-08  tail 5.4e-08 7.6e-06 7.9e-08  plain 3.9e-08 7.5e-06 7.7e-08
  running_mean    offset 3.4e-07 3.4e-05 2.6e-07  outlier 5.6e-08 6.3e-06 7.0e-08  tail 1.2e-08 3.1e-06 2.3e-08  plain 7.9e-09 2.4e-06 1.0e-08
  running_var     offset 1.7e-05 6.8e-05 8.0e-08  outlier 9.4e-07 7.9e-05 9.3e-07  tail 6.5e-08 1.5e-05 6.5e-08  plain 5.2e-08 1.6e-05 8.8e-08
  y               offset 4.6e-03 1.8e-02 9.0e-06  outlier 3.8e-07 8.4e-05 6.7e-07  tail 4.2e-07 6.3e-05 4.7e-07  plain 4.3e-07 6.8e-05 8.1e-07
  dx              const 1.9e-05 2.8e-03 1.2e-05  offset 1.8e-02 7.1e-02 1.3e-05  outlier 8.4e-08 3.0e-05 5.1e-08  tail 3.4e-07 8.3e-05 3.4e-07  plain 3.3e-07 6.8e-05 3.2e-07
  dgamma          const 0.0e+00 1.6e-04 0.0e+00  offset 1.2e-02 4.8e-02 1.3e-04  outlier 1.3e-06 3.3e-04 2.6e-06  tail 1.0e-06 4.4e-04 1.3e-06  plain 2.9e-06 3.8e-04 1.8e-06
  dbeta           const 0.0e+00 8.0e-04 0.0e+00  offset 1.7e-06 6.3e-04 1.7e-06  outlier 1.5e-06 3.5e-04 1.1e-06  tail 1.4e-06 3.6e-04 1.2e-06  plain 1.1e-06 3.5e-04 1.1e-06
  dgamma_r        const 0.0e+00 1.4e-04 0.0e+00  offset 1.2e-02 4.7e-02 9.7e-05  outlier 1.9e-06 2.9e-04 2.4e-06  tail 1.0e-06 3.9e-04 1.3e-06  plain 2.8e-06 3.6e-04 1.9e-06
  dbeta_r         const 0.0e+00 6.2e-04 0.0e+00  offset 1.3e-06 5.1e-04 7.5e-07  outlier 1.3e-06 3.2e-04 7.3e-07  tail 1.2e-06 2.8e-04 9.1e-07  plain 7.2e-07 3.7e-04 9.5e-07
syncbn module two-slices
  mean            offset 8.4e-06 3.2e-04 7.4e-07  outlier 7.6e-07 2.4e-05 2.0e-07  tail 6.1e-08 5.2e-06 6.1e-08  plain 1.4e-07 6.1e-06 2.0e-08
  invstd          offset 3.5e-07 4.1e-05 1.3e-07  outlier 5.1e-09 2.7e-06 5.1e-09  tail 1.8e-08 8.1e-06 1.8e-08  plain 5.4e-09 6.0e-06 5.4e-09
  running_mean    offset 3.6e-07 3.3e-05 1.2e-07  outlier 3.7e-08 4.4e-06 2.3e-08  tail 2.7e-09 2.5e-06 2.7e-09  plain 2.7e-09 1.5e-06 2.7e-09
  running_var     offset 4.1e-05 1.6e-04 3.8e-08  outlier 3.2e-08 4.5e-05 5.1e-07  tail 1.1e-08 1.4e-05 1.1e-08  plain 3.7e-08 9.5e-06 3.7e-08
  y               tail 3.7e-07 7.2e-05 2.4e-07  plain 3.0e-07 7.5e-05 3.0e-07
  dx              const 6.8e-06 2.6e-03 9.8e-06  tail 3.3e-07 6.5e-05 2.5e-07  plain 1.3e-07 4.2e-05 9.3e-08
  dgamma          const 0.0e+00 3.0e-03 0.0e+00  offset 4.0e-01 1.6e+00 6.5e-05  outlier 1.2e-05 3.9e-03 3.7e-06  tail 2.1e-05 5.5e-03 1.9e-05  plain 1.2e-05 5.3e-03 2.0e-05
  dbeta           const 0.0e+00 2.2e-01 0.0e+00  offset 7.7e-06 3.5e-03 1.7e-05  outlier 4.8e-06 4.0e-03 9.6e-07  tail 4.9e-06 6.2e-03 4.9e-06  plain 2.2e-05 7.3e-03 8.7e-06
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R
from branch_replay import pool_code_to_index, train_pre_mask

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MOM, EPS = 0.1, 1e-5
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops as _ops
    return _ops


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _floor(name, n):
    """(rtol, atol) the existing tests of these paths already allow on the suite's plain input"""
    if name in ("y", "yp"):
        return 1e-5, 2e-5
    if name in ("mean", "invstd", "running_mean", "running_var"):
        return R.STAT_FLOOR  # 1e-5, 1e-6: the host test of eeadv.syncbn's merge takes the same pair
    if name in ("dgamma", "dbeta"):
        return 2e-5, 2e-5 * max(1.0, float(n) ** 0.5)
    return 2e-5, 2e-5  # dx, dresidual


def _chan_max(t):
    return t.amax((0, 2, 3)) if t.dim() == 4 else t


def _bounded(case, name, got, ref, stock, ref_stock, kinds, n, skip=(), chan_rel=None):
    """|got - ref| <= max(4 * the stock kernel's error on that channel, floor), element by element, on every channel not in `skip`.
    The floor is _floor's rtol / atol, or - chan_rel - that fraction of the channel's own largest reference entry."""
    assert bool(torch.isfinite(got).all()), "%s %s: NaN / inf" % (case, name)
    ref, ref_stock = ref.to(DEV), ref_stock.to(DEV)
    err = (got.detach().double() - ref).abs()
    serr = _chan_max((stock.detach().double() - ref_stock).abs())
    if chan_rel is not None:
        floor = (chan_rel * _chan_max(ref.abs())).view(1, -1, 1, 1)
    else:
        rtol, atol = _floor(name, n)
        floor = atol + rtol * ref.abs()
    bound = torch.maximum(4.0 * (serr.view(1, -1, 1, 1) if err.dim() == 4 else serr), floor).expand_as(err)
    ok = _chan_max((err > bound).to(torch.int32)) == 0
    kerr, kbound = _chan_max(err), _chan_max(bound)
    for kind in sorted(set(kinds)):
        idx = [c for c, k in enumerate(kinds) if k == kind and c not in skip]
        if idx:
            print("BNHARD %s | %s | %s | kernel %.2e | stock %.2e | bound %.2e" % (case, name, kind, float(kerr[idx].max()), float(serr[idx].max()),
                                                                             float(kbound[idx].max())))
    bad = [c for c in range(len(kinds)) if c not in skip and not bool(ok[c])]
    assert not bad, "%s %s: channels %s (%s) exceed the bound: kernel %s, stock %s, bound %s" % (
        case, name, bad, [kinds[c] for c in bad], kerr[bad].tolist(), serr[bad].tolist(), kbound[bad].tolist())


def _moved(r0, value):
    """(1 - momentum) * r0 + momentum * value, in the kernels' fp32 steps"""
    m = F32(MOM)
    return (F32(1.0) - m) * r0.cpu().numpy().astype(F32) + m * F32(value)


INVSTD0 = F32(1.0) / np.sqrt(F32(0.0) + F32(EPS))


def _exact_stats(case, chans, constant, sm, si, rm, rv, rm0, rv0):
    """a channel whose every value is `constant`: mean exact, M2 exactly 0"""
    for c in chans:
        assert float(sm[c]) == constant, "%s: save_mean[%d] = %r" % (case, c, float(sm[c]))
        assert F32(float(si[c])) == INVSTD0, "%s: save_invstd[%d] = %r, fp32 1/sqrtf(eps) = %r" % (case, c, float(si[c]), float(INVSTD0))
        assert F32(float(rm[c])) == _moved(rm0, constant)[c], "%s: running_mean[%d]" % (case, c)
        assert F32(float(rv[c])) == _moved(rv0, 0.0)[c], "%s: running_var[%d]" % (case, c)


def _mask_agrees(case, y32, pre64, gamma):
    live = (gamma != 0).nonzero().flatten().tolist()
    clear = pre64[:, live].abs() > R.TIE_BAND
    same = (y32[:, live] > 0) == (pre64[:, live] > 0)
    assert bool((same | ~clear).all()), "%s: the fp32 ReLU mask differs from the float64 one outside the tie band at %d elements" % (
        case, int((~same & clear).sum()))


def _stock_bn(c, training, res, res_in=None, relu=True):
    """torch's stock fp32 batch_norm / autograd on the same tensors, with ITS ReLU branch, and the float64 bar on that branch"""
    x, w, b = (c[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    r = c["residual"].clone().requires_grad_(True) if res else None
    rm, rv = c["rm"].clone(), c["rv"].clone()
    s = x if res_in is None else x + res_in
    pre = F.batch_norm(s, rm, rv, w, b, training, MOM, EPS)
    if res:
        pre = pre + r
    y = F.relu(pre) if relu else pre
    g = torch.autograd.grad(y, [x, w, b] + ([r] if res else []), c["dy"])
    out = {"y": y.detach(), "running_mean": rm, "running_var": rv, "dx": g[0], "dgamma": g[1], "dbeta": g[2], "dresidual": g[3] if res else None}
    if training:  # the batch statistics as the stock kernel forms them: momentum 1 on zeroed running statistics
        m1, v1 = torch.zeros_like(rm), torch.zeros_like(rv)
        F.batch_norm(s.detach(), m1, v1, None, None, True, 1.0, EPS)
        n = s.numel() // s.shape[1]
        out["mean"] = m1
        out["invstd"] = (1.0 / torch.sqrt(v1.double() * ((n - 1.0) / n) + R.eps32(EPS))).float()
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, training, res_in=res_in, residual=c["residual"] if res else None,
                     relu=relu, dy=c["dy"], mask=(y > 0) if relu else None)
    return out, ref


def _to_dev(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _verify(case, c, got, ref, training, res, exact_y, exact_dx, res_in=None):
    """the assertions of the module header on one BatchNorm's results `got` (a dict with bn_ref64's keys)"""
    kinds, gamma, beta = c["kinds"], c["gamma"], c["beta"]
    C = len(kinds)
    n = c["x"].numel() // C
    stock, ref_stock = _stock_bn(c, training, res, res_in)
    const = [i for i, k in enumerate(kinds) if k == "const"] if training else []
    zero_gamma = (gamma == 0).nonzero().flatten().tolist()
    if training:
        _exact_stats(case, const, R.CONST, got["mean"], got["invstd"], got["running_mean"], got["running_var"], c["rm"], c["rv"])
    want_flat = torch.relu(beta.view(1, -1, 1, 1) + c["residual"]) if res else torch.relu(beta).view(1, -1, 1, 1).expand_as(c["x"])
    flat = sorted(set(const) | set(zero_gamma)) if exact_y else []
    if flat:
        assert torch.equal(got["y"][:, flat], want_flat[:, flat]), "%s: y != relu(beta%s) on the constant / gamma == 0 channels" % (case, " + residual" if res else "")
    if exact_y and not res:
        for ch in zero_gamma:
            assert bool(((got["y"][:, ch] > 0) == bool(beta[ch] > 0)).all()), "%s: gamma == 0 channel %d does not follow beta > 0" % (case, ch)
    still = sorted(set(zero_gamma) | (set(const) if exact_dx else set()))
    if got.get("dx") is not None and still:
        assert bool((got["dx"][:, still] == 0).all()), "%s: dx != 0 on channels %s" % (case, still)
    stat_names = ["mean", "invstd", "running_mean", "running_var"] if training else []

    def bounded(names):
        for name in names:
            if got.get(name) is not None:
                skip = const if name in stat_names else (flat if name == "y" else (still if name == "dx" else ()))
                _bounded(case, name, got[name], ref[name], stock[name], ref_stock[name], kinds, n, skip)
    bounded(stat_names)  # before the masks: a wrong statistic is the cause, a flipped branch its symptom
    _mask_agrees(case, got["y"], ref["pre"].to(DEV), gamma)
    bounded(["y", "dx", "dresidual", "dgamma", "dbeta"])


# ---- ee_bn_act_fwd_f32 / ee_bn_act_bwd2_f32: every dispatch branch -------------------------------------------------------------------------
def _misaligned(t):
    """the same values in a contiguous view that starts one float into its storage (4 bytes past a 16-byte boundary)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _act_fwd(x, res, c, training, workspace):
    from eeadv import _native as N
    from eeadv.ops import _stream
    B, C, H, W = x.shape
    y, sm, si = torch.empty(x.shape, device=DEV), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm, rv = c["rm"].clone(), c["rv"].clone()
    nws = N.lib.ee_bn_workspace_floats(B, C, H * W)
    ws = torch.empty(nws, device=DEV) if (workspace and nws) else None
    N.check(N.lib.ee_bn_act_fwd_f32(_p(x), _p(res), _p(c["gamma"]), _p(c["beta"]), _p(rm), _p(rv), MOM, EPS, int(training), 1, _p(y),
                                    _p(sm) if training else None, _p(si) if training else None, _p(ws), B, C, H * W, _stream()), "ee_bn_act_fwd_f32")
    return {"y": y, "mean": sm if training else None, "invstd": si if training else None, "running_mean": rm, "running_var": rv}


def _act_bwd(dy, y, x, c, fw, training, want_dres, workspace, beta=None):
    from eeadv import _native as N
    from eeadv.ops import _stream
    B, C, H, W = x.shape
    dx, dres = torch.empty(x.shape, device=DEV), (torch.empty(x.shape, device=DEV) if want_dres else None)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    nws = N.lib.ee_bn_workspace_floats(B, C, H * W)
    ws = torch.empty(nws, device=DEV) if (workspace and nws) else None
    N.check(N.lib.ee_bn_act_bwd2_f32(_p(dy), None, _p(y), _p(x), _p(c["gamma"]), _p(beta), _p(fw["mean"]), _p(fw["invstd"]), _p(c["rm"]), _p(c["rv"]),
                                     EPS, int(training), 1, _p(dx), _p(dres), _p(dg), _p(db), _p(ws), B, C, H * W, _stream()), "ee_bn_act_bwd2_f32")
    return {"dx": dx, "dresidual": dres, "dgamma": dg, "dbeta": db}


ACT_PATHS = list(R.BN_ACT_CASES) + ["vector<1024,4>-no-workspace", "alignment-fallback"]


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("path", ACT_PATHS)
def test_bn_act_every_dispatch_branch(path, training, res):
    from eeadv import _native as N
    key = {"vector<1024,4>-no-workspace": "split-4-slices", "alignment-fallback": "cached<256,7>"}.get(path, path)
    shape, seed = R.BN_ACT_CASES[key]
    c = _to_dev(R.hard_case(shape, seed))
    workspace = path != "vector<1024,4>-no-workspace"
    B, C, H, W = shape
    if key == "split-4-slices":  # the shape the split pair takes in four slices, the last one shorter
        quads = B * H * W // 4
        assert N.lib.ee_bn_workspace_floats(B, C, H * W) == C * 4 * 2 and quads % 4 != 0 and quads > 7 * 1024
    x, dy = c["x"], c["dy"]
    if path == "alignment-fallback":
        x, dy = _misaligned(x), _misaligned(dy)
    r = c["residual"] if res else None
    fw = _act_fwd(x, r, c, training, workspace)
    again = _act_fwd(x, r, c, training, workspace)
    for k, v in fw.items():
        assert v is None or torch.equal(v, again[k]), "%s: %s differs between two calls" % (path, k)
    bw = _act_bwd(dy, fw["y"], x, c, fw, training, res, workspace)
    for k, v in _act_bwd(dy, fw["y"], x, c, fw, training, res, workspace).items():
        assert v is None or torch.equal(v, bw[k]), "%s: %s differs between two calls" % (path, k)
    if not res:  # the mask recomputed from x, gamma, beta: the bits of the mask read from y
        for k, v in _act_bwd(dy, None, x, c, fw, training, False, workspace, beta=c["beta"]).items():
            assert v is None or torch.equal(v, bw[k]), "%s: %s with the mask from x differs from the mask from y" % (path, k)
    got = dict(fw, **bw)
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, training, residual=r, relu=True, dy=c["dy"], mask=fw["y"] > 0)
    _verify("bn_act %s %s%s" % (path, "train" if training else "eval", " +res" if res else ""), c, got, ref, training, res, True, not res)


# ---- ee_bn_dual_*: relu(bn_a(xa) + bn_b(xb)), different kinds on the two sides ---------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_bn_dual_on_hard_channels(ops, training):
    shape, seed = R.BN_DUAL_CASE
    a, b = _to_dev(R.hard_case(shape, seed)), _to_dev(R.hard_case(shape, seed + 1, roll=2))
    assert ops.bn_dual_supported(a["x"]) and a["kinds"] != b["kinds"]
    C, n = shape[1], shape[0] * shape[2] * shape[3]

    def run():
        st = [a["rm"].clone(), a["rv"].clone(), b["rm"].clone(), b["rv"].clone()]
        y, sv = ops.bn_dual_fwd(a["x"], b["x"], (a["gamma"], a["beta"], st[0], st[1], MOM, EPS), (b["gamma"], b["beta"], st[2], st[3], MOM, EPS), training)
        g = ops.bn_dual_bwd(a["dy"], None, y, a["x"], b["x"], a["gamma"], b["gamma"], sv, a["rm"], a["rv"], b["rm"], b["rv"], EPS, EPS, training)
        return [y] + list(sv) + st + list(g)
    one, two = run(), run()
    for i, (u, v) in enumerate(zip(one, two)):
        assert u is None or torch.equal(u, v), "bn_dual: result %d differs between two calls" % i
    y, sma, sia, smb, sib, rma, rva, rmb, rvb, dxa, dxb, dga, dba, dgb, dbb = one
    # the float64 bar on the kernel's branch: side b without a ReLU, its result the residual of side a
    mask = y > 0
    rb = R.bn_ref64(b["x"], b["gamma"], b["beta"], b["rm"], b["rv"], MOM, EPS, training, relu=False)
    ra = R.bn_ref64(a["x"], a["gamma"], a["beta"], a["rm"], a["rv"], MOM, EPS, training, residual=rb["y"], relu=True, dy=a["dy"], mask=mask)
    rb = R.bn_ref64(b["x"], b["gamma"], b["beta"], b["rm"], b["rv"], MOM, EPS, training, relu=False, dy=ra["dresidual"])
    # stock, on its own branch
    ts = {k: [s[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta")] for k, s in (("a", a), ("b", b))}
    srun = [a["rm"].clone(), a["rv"].clone(), b["rm"].clone(), b["rv"].clone()]
    qb = F.batch_norm(ts["b"][0], srun[2], srun[3], ts["b"][1], ts["b"][2], training, MOM, EPS)
    ys = F.relu(F.batch_norm(ts["a"][0], srun[0], srun[1], ts["a"][1], ts["a"][2], training, MOM, EPS) + qb)
    sg = torch.autograd.grad(ys, ts["a"] + ts["b"], a["dy"])
    sb = R.bn_ref64(b["x"], b["gamma"], b["beta"], b["rm"], b["rv"], MOM, EPS, training, relu=False)
    sa = R.bn_ref64(a["x"], a["gamma"], a["beta"], a["rm"], a["rv"], MOM, EPS, training, residual=sb["y"], relu=True, dy=a["dy"], mask=ys > 0)
    sb = R.bn_ref64(b["x"], b["gamma"], b["beta"], b["rm"], b["rv"], MOM, EPS, training, relu=False, dy=sa["dresidual"])
    mode = "train" if training else "eval"
    _mask_agrees("bn_dual " + mode, y, ra["pre"].to(DEV), torch.ones(C))  # a gamma_a == 0 channel still carries side b
    for side, s, got, ref, stk, sref in (
            ("a", a, {"mean": sma, "invstd": sia, "running_mean": rma, "running_var": rva, "y": y, "dx": dxa, "dgamma": dga, "dbeta": dba}, ra,
             {"running_mean": srun[0], "running_var": srun[1], "y": ys.detach(), "dx": sg[0], "dgamma": sg[1], "dbeta": sg[2]}, sa),
            ("b", b, {"mean": smb, "invstd": sib, "running_mean": rmb, "running_var": rvb, "dx": dxb, "dgamma": dgb, "dbeta": dbb}, rb,
             {"running_mean": srun[2], "running_var": srun[3], "dx": sg[3], "dgamma": sg[4], "dbeta": sg[5]}, sb)):
        case = "bn_dual %s side %s" % (mode, side)
        const = [i for i, k in enumerate(s["kinds"]) if k == "const"] if training else []
        if training:
            _exact_stats(case, const, R.CONST, got["mean"], got["invstd"], got["running_mean"], got["running_var"], s["rm"], s["rv"])
            m1, v1 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            F.batch_norm(s["x"], m1, v1, None, None, True, 1.0, EPS)
            stk = dict(stk, mean=m1, invstd=(1.0 / torch.sqrt(v1.double() * ((n - 1.0) / n) + R.eps32(EPS))).float())
        zero_gamma = (s["gamma"] == 0).nonzero().flatten().tolist()
        assert bool((got["dx"][:, zero_gamma] == 0).all()), case + ": dx != 0 where gamma == 0"
        for name in (["mean", "invstd", "running_mean", "running_var"] if training else []) + ["y", "dx", "dgamma", "dbeta"]:
            if name in got:
                _bounded(case, name, got[name], ref[name], stk[name], sref[name], s["kinds"], n, const if name in ("mean", "invstd", "running_mean", "running_var") else ())


# ---- ee_bn_sum_act_*: the statistics are those of x + res -------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("path", list(R.BN_SUM_CASES))
def test_bn_sum_act_on_hard_channels(ops, path, training):
    shape, seed = R.BN_SUM_CASES[path]
    c = R.hard_case(shape, seed)
    x, res = R.split_sum(c["x"], seed)
    c = _to_dev(dict(c, x=x))
    res = res.to(DEV)
    assert ops.bn_sum_act_supported(c["x"])

    def run(mask_from_x):
        rm, rv = c["rm"].clone(), c["rv"].clone()
        y, s, sm, si = ops.bn_sum_act_fwd(c["x"], res, c["gamma"], c["beta"], rm, rv, MOM, EPS, training, True)
        ds, dg, db = ops.bn_sum_act_bwd(c["dy"], None, None if mask_from_x else y, s, c["gamma"], c["beta"], sm, si, c["rm"], c["rv"], EPS, training, True)
        return {"y": y, "s": s, "mean": sm, "invstd": si, "running_mean": rm, "running_var": rv, "dx": ds, "dgamma": dg, "dbeta": db}
    got, again, from_x = run(False), run(False), run(True)
    for k, v in got.items():
        assert v is None or (torch.equal(v, again[k]) and torch.equal(v, from_x[k])), "bn_sum_act %s: %s differs between two calls / mask forms" % (path, k)
    assert torch.equal(got["s"], c["x"] + res)
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, training, res_in=res, relu=True, dy=c["dy"], mask=got["y"] > 0)
    _verify("bn_sum_act %s %s" % (path, "train" if training else "eval"), c, got, ref, training, False, True, True, res_in=res)


# ---- ee_bn_relu_pool_*: own statistics (the split pair's partials), the _xa pair, and the stem convolution's tiles -------------------------
def _pool_scatter(vals, idx, shape):
    B, C, H, W = shape
    full = torch.zeros(B, C, H * W, dtype=vals.dtype, device=vals.device)
    full.scatter_add_(2, idx.reshape(B, C, -1), vals.reshape(B, C, -1))
    return full.view(shape)


def _pool_bar(c, training, yp, idx, dyp):
    """bn_ref64 behind a 3x3 / stride 2 pool whose argmax (flat indices `idx`) and ReLU branch (yp > 0 at the argmax) are held fixed"""
    shape = c["x"].shape
    dy_full = _pool_scatter(dyp.double(), idx, shape)
    mask = _pool_scatter((yp > 0).double(), idx, shape) > 0
    r = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, training, relu=True, dy=dy_full, mask=mask)
    r["yp"] = F.max_pool2d(r["y"], 3, 2, 1)
    return r


def _pool_stock(c, training, dyp):
    x, w, b = (c[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = c["rm"].clone(), c["rv"].clone()
    yp, idx = F.max_pool2d(F.relu(F.batch_norm(x, rm, rv, w, b, training, MOM, EPS)), 3, 2, 1, return_indices=True)
    g = torch.autograd.grad(yp, [x, w, b], dyp)
    out = {"yp": yp.detach(), "running_mean": rm, "running_var": rv, "dx": g[0], "dgamma": g[1], "dbeta": g[2]}
    if training:
        m1, v1 = torch.zeros_like(rm), torch.zeros_like(rv)
        F.batch_norm(c["x"], m1, v1, None, None, True, 1.0, EPS)
        n = x.numel() // x.shape[1]
        out["mean"], out["invstd"] = m1, (1.0 / torch.sqrt(v1.double() * ((n - 1.0) / n) + R.eps32(EPS))).float()
    return out, _pool_bar(c, training, yp.detach(), idx, dyp)


def _verify_pool(case, c, got, training, dyp, constant, const):
    kinds, gamma, beta = c["kinds"], c["gamma"], c["beta"]
    n = c["x"].numel() // len(kinds)
    ref = _pool_bar(c, training, got["yp"], pool_code_to_index(got["code"], c["x"].shape[3]), dyp)
    stock, ref_stock = _pool_stock(c, training, dyp)
    const = const if training else []
    zero_gamma = (gamma == 0).nonzero().flatten().tolist()
    if training:
        _exact_stats(case, const, constant, got["mean"], got["invstd"], got["running_mean"], got["running_var"], c["rm"], c["rv"])
    flat = sorted(set(const) | set(zero_gamma))
    assert torch.equal(got["yp"][:, flat], torch.relu(beta).view(1, -1, 1, 1).expand_as(got["yp"])[:, flat]), case + ": pooled y != relu(beta) on the flat channels"
    if got.get("dx") is not None:
        assert bool((got["dx"][:, zero_gamma] == 0).all()), case + ": dx != 0 where gamma == 0"
    # the mask behind the pool: a window's largest float64 pre-activation outside the tie band decides whether the pooled fp32 value is open
    _mask_agrees(case + " (pooled)", got["yp"], F.max_pool2d(ref["pre"].to(DEV), 3, 2, 1), gamma)
    stat_names = ["mean", "invstd", "running_mean", "running_var"] if training else []
    for name in stat_names + ["yp", "dx", "dgamma", "dbeta"]:
        if got.get(name) is not None:
            _bounded(case, name, got[name], ref[name], stock[name], ref_stock[name], kinds, n, const if name in stat_names else (flat if name == "yp" else ()))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("path", list(R.BN_POOL_CASES))
def test_bn_relu_pool_own_statistics_on_hard_channels(ops, path, training):
    shape, seed = R.BN_POOL_CASES[path]
    c = _to_dev(R.hard_case(shape, seed))
    assert ops.bn_relu_pool_supported(c["x"])
    OH, OW = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    dyp = c["dy"][:, :, :OH, :OW].contiguous()

    def run(xa):
        rm, rv = c["rm"].clone(), c["rv"].clone()
        out = ops.bn_relu_pool_fwd(c["x"], c["gamma"], c["beta"], rm, rv, MOM, EPS, training, want_x_argmax=xa)
        yp, code, sm, si = out[:4]
        dx, dg, db = ops.bn_relu_pool_bwd(dyp, code, c["x"], c["gamma"], c["beta"], sm, si, c["rm"], c["rv"], EPS, training, x_argmax=out[4] if xa else None)
        return {"yp": yp, "code": code, "mean": sm, "invstd": si, "running_mean": rm, "running_var": rv, "dx": dx, "dgamma": dg, "dbeta": db,
                "xa": out[4] if xa else None}
    got, again, pooled = run(False), run(False), run(True)
    for k, v in got.items():
        assert v is None or torch.equal(v, again[k]), "bn_relu_pool %s: %s differs between two calls" % (path, k)
    for k in ("yp", "code", "mean", "invstd", "running_mean", "running_var"):
        assert got[k] is None or torch.equal(got[k], pooled[k]), "bn_relu_pool %s: the _xa forward's %s differs" % (path, k)
    idx = pool_code_to_index(got["code"], shape[3])
    assert torch.equal(pooled["xa"], c["x"].flatten(2).gather(2, idx.flatten(2)).view_as(pooled["xa"]))
    const = [i for i, k in enumerate(c["kinds"]) if k == "const"]
    mode = "train" if training else "eval"
    _verify_pool("bn_relu_pool %s %s" % (path, mode), c, got, training, dyp, R.CONST, const)
    _verify_pool("bn_relu_pool_xa %s %s" % (path, mode), c, pooled, training, dyp, R.CONST, const)


def _conv_kinds(C):
    return ["zero-filter" if i in R.ZERO_FILTER_CHANNELS else "conv-out" for i in range(C)]


def test_bn_relu_pool_merges_the_stem_convolutions_unequal_tiles(ops):
    xs, K, seed = R.STEM_CASE
    x, w = (t.to(DEV) for t in R.shaped_conv_operands(xs, (K, 3, 7, 7), seed, 147))
    assert ops.stem7x7s2_fwd_supported(x, w)
    raw, st = ops.stem7x7s2_fwd(x, w, True)
    counts = st[:, :, 2]
    assert len(torch.unique(counts[counts > 0])) > 1, "the case is meant to merge tiles of unequal counts"
    zf = list(R.ZERO_FILTER_CHANNELS)
    assert bool((raw[:, zf] == 0).all())
    gamma, beta = (t.to(DEV) for t in R.hard_affine(K))
    rm0, rv0 = (t.to(DEV) for t in R.hard_running(K))
    g = torch.Generator().manual_seed(seed)
    dyp = torch.randn(xs[0], K, 3, 16, generator=g).to(DEV)
    c = {"x": raw, "gamma": gamma, "beta": beta, "rm": rm0, "rv": rv0, "kinds": _conv_kinds(K)}

    def run():
        rm, rv = rm0.clone(), rv0.clone()
        yp, code, sm, si = ops.bn_relu_pool_fwd(raw, gamma, beta, rm, rv, MOM, EPS, True, conv_stats=st)
        dx, dg, db = ops.bn_relu_pool_bwd(dyp, code, raw, gamma, beta, sm, si, None, None, EPS, True)
        return {"yp": yp, "code": code, "mean": sm, "invstd": si, "running_mean": rm, "running_var": rv, "dx": dx, "dgamma": dg, "dbeta": db}
    got, again = run(), run()
    for k, v in got.items():
        assert torch.equal(v, again[k]), "bn_relu_pool with conv_stats: %s differs between two calls" % k
    _verify_pool("bn_relu_pool conv_stats", c, got, True, dyp, 0.0, zf)


# ---- the convolution producers: statistics written next to the raw output, merged by ee_wino3x3_bn_train_pre_f32 ------------------------
def _verify_train_pre(case, ops, raw, stats, cnt, w2, seed):
    """`raw` [B, C, H, H] is the producer's own fp32 output (the convolution itself is pinned elsewhere): the bar is float64 statistics of it"""
    from eeadv import functional as Fn
    B, C, H = raw.shape[0], raw.shape[1], raw.shape[2]
    n = B * H * H
    gamma, beta = (t.to(DEV) for t in R.hard_affine(C))
    rm0, rv0 = (t.to(DEV) for t in R.hard_running(C))
    u2 = Fn.wino_sets(w2)[0]
    kinds = _conv_kinds(C)
    zf = list(R.ZERO_FILTER_CHANNELS)
    assert bool((raw[:, zf] == 0).all()), case + ": a zero filter did not give a zero channel"

    def run():
        rm, rv = rm0.clone(), rv0.clone()
        y, sm, si = ops.wino3x3_bn_train_pre(raw, stats, cnt, gamma, beta, EPS, MOM, rm, rv, u2)
        return {"conv": y, "mean": sm, "invstd": si, "running_mean": rm, "running_var": rv}
    got, again = run(), run()
    for k, v in got.items():
        assert torch.equal(v, again[k]), "%s: %s differs between two calls" % (case, k)
    _exact_stats(case, zf, 0.0, got["mean"], got["invstd"], got["running_mean"], got["running_var"], rm0, rv0)
    ref = R.bn_ref64(raw, gamma, beta, rm0, rv0, MOM, EPS, True, relu=True)
    # the branch the consumer opens on its own statistics (branch_replay.train_pre_mask: the fp32 expression of ee_fuse.hpp's train_bn_apply)
    opened = train_pre_mask(raw, got["mean"], got["invstd"], gamma, beta)
    _mask_agrees(case, opened.float(), ref["pre"].to(DEV), gamma)
    for ch in (gamma == 0).nonzero().flatten().tolist():
        assert bool((opened[:, ch] == bool(beta[ch] > 0)).all()), "%s: gamma == 0 channel %d does not follow beta > 0" % (case, ch)
    srm, srv, m1, v1 = rm0.clone(), rv0.clone(), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    sy = F.relu(F.batch_norm(raw, srm, srv, gamma, beta, True, MOM, EPS))
    F.batch_norm(raw, m1, v1, None, None, True, 1.0, EPS)
    stock = {"mean": m1, "invstd": (1.0 / torch.sqrt(v1.double() * ((n - 1.0) / n) + R.eps32(EPS))).float(), "running_mean": srm, "running_var": srv}
    for name in ("mean", "invstd", "running_mean", "running_var"):
        _bounded(case, name, got[name], ref[name], stock[name], ref[name], kinds, n, zf)
    # the consumer's own result: conv2 of the activations, the bar in float64 throughout
    want = F.conv2d(ref["y"], w2.double(), None, 1, 1)
    _bounded(case, "conv2(relu(bn))", got["conv"], want, F.conv2d(sy, w2, None, 1, 1), want, ["conv-out"] * w2.shape[0], n, (), chan_rel=2e-5)
    return got, gamma, beta


@pytest.mark.parametrize("H", sorted(R.WINO_CASES))
def test_wino_statistics_feed_the_train_mode_consumer(ops, H):
    from eeadv import functional as Fn
    seed = R.WINO_CASES[H]
    C = 32  # producer and consumer take any multiple of 32 channels up to 256 on 4 x 4, 8 x 8 and 16 x 16 maps (ee_wino.hip: wino_check, WN_MAX_KC_TRAIN)
    x, w1 = (t.to(DEV) for t in R.shaped_conv_operands((3, C, H, H), (C, C, 3, 3), seed, 9 * C))
    w2 = (torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(seed + 1)) * (2.0 / (9 * C)) ** 0.5).to(DEV)
    u1, u1b = Fn.wino_sets(w1)
    raw, stats = ops.wino3x3_stats(x, u1)
    assert torch.equal(raw, ops.wino3x3(x, u1))
    got, gamma, beta = _verify_train_pre("wino_stats H=%d C=%d" % (H, C), ops, raw, stats, H * H, w2, seed)
    if H != 16:
        return
    # the backward across the boundary (16 x 16 maps): the producer's per-image sums open the mask the forward opened
    u2b = Fn.wino_sets(w2)[1]
    dc2 = torch.randn(raw.shape, generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    d_a1, sums = ops.wino3x3_bwd_sums(dc2, u2b, raw, got["mean"], got["invstd"], gamma, beta)
    assert torch.equal(d_a1, ops.wino3x3(dc2, u2b))
    mask = train_pre_mask(raw, got["mean"], got["invstd"], gamma, beta)
    dz = torch.where(mask, d_a1, torch.zeros_like(d_a1)).double()
    xhat = ((raw - got["mean"].view(1, -1, 1, 1)) * got["invstd"].view(1, -1, 1, 1)).double()
    # a 256-term fp32 sum in any order is within 256 * 2^-24 of the sum of magnitudes; one wrongly opened element moves it by that element
    u = 256 * 2.0 ** -24
    e0 = (sums[:, :, 0].double() - dz.sum((2, 3)).t()).abs()
    e1 = (sums[:, :, 1].double() - (dz * xhat).sum((2, 3)).t()).abs()
    assert bool((e0 <= u * dz.abs().sum((2, 3)).t() + 1e-30).all()) and bool((e1 <= 2 * u * (dz * xhat).abs().sum((2, 3)).t() + 1e-30).all())
    dx = ops.wino3x3_bn_train_bwd_pre(d_a1, raw, sums, H * H, got["mean"], got["invstd"], gamma, beta, u1b)
    # against the unfused kernels on the same saved statistics: ee_bn_act_bwd2_f32 with the mask from y, then the convolution
    y_full = torch.relu((raw - got["mean"].view(1, -1, 1, 1)) * (got["invstd"] * gamma).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1))
    d_c1 = ops.bn_act_bwd(d_a1, y_full, raw, gamma, got["mean"], got["invstd"], None, None, EPS, True, True, True, False, False)[0]
    from_x = ops.bn_act_bwd(d_a1, None, raw, gamma, got["mean"], got["invstd"], None, None, EPS, True, True, True, False, False, None, beta)[0]
    assert torch.equal(d_c1, from_x) and torch.equal(mask, y_full > 0)
    unfused = ops.wino3x3(d_c1, u1b)
    worst = ((dx - unfused).abs().amax((0, 2, 3)) / unfused.abs().amax((0, 2, 3))).max()  # test_gpu_trainfuse.py's 2e-5, of each result channel's own largest entry
    assert float(worst) <= 2e-5, "the fused backward differs from ee_bn_act_bwd2_f32 | ee_wino3x3_f32 by %.3e of a channel's largest entry" % float(worst)
    # float64 bar on that branch, the convolution in float64 too; the stock side is torch's fp32 autograd and convolution
    r = R.bn_ref64(raw, gamma, beta, None, None, MOM, EPS, True, relu=True, dy=d_a1, mask=mask)
    want = F.conv_transpose2d(r["dx"], w1.double(), None, 1, 1)
    rs = raw.clone().requires_grad_(True)
    ys = F.relu(F.batch_norm(rs, None, None, gamma, beta, True, MOM, EPS))
    (sdx,) = torch.autograd.grad(ys, [rs], d_a1)
    rstock = R.bn_ref64(raw, gamma, beta, None, None, MOM, EPS, True, relu=True, dy=d_a1, mask=ys > 0)
    _bounded("wino_bwd_pre H=16", "conv1^T(bn_bwd)", dx, want, F.conv_transpose2d(sdx, w1, None, 1, 1), F.conv_transpose2d(rstock["dx"], w1.double(), None, 1, 1),
             ["conv-out"] * w1.shape[1], 3 * H * H, (), chan_rel=2e-5)
    d_again, s_again = ops.wino3x3_bwd_sums(dc2, u2b, raw, got["mean"], got["invstd"], gamma, beta)
    assert torch.equal(s_again, sums) and torch.equal(ops.wino3x3_bn_train_bwd_pre(d_again, raw, s_again, H * H, got["mean"], got["invstd"], gamma, beta, u1b), dx)


@pytest.mark.parametrize("mt", ["222111", "111222"])
@pytest.mark.parametrize("H", sorted(R.PAIR_CASES))
def test_pair_statistics_feed_the_train_mode_consumer(ops, monkeypatch, H, mt):
    from eeadv import functional as Fn
    monkeypatch.setenv("EEADV_S2_MT", mt)
    seed = R.PAIR_CASES[H]
    x, w3 = (t.to(DEV) for t in R.shaped_conv_operands((3, 32, H, H), (64, 32, 3, 3), seed, 9 * 32))
    g = torch.Generator().manual_seed(seed + 1)
    wd = (torch.randn(64, 32, 1, 1, generator=g) * (2.0 / 32) ** 0.5).to(DEV)
    w2 = (torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (9 * 64)) ** 0.5).to(DEV)
    w10 = Fn._dense_weight(w3, "s2p_f", wd)
    y3, y1, stats, cnt = ops.conv3x3s2_pair_stats_fwd(x, w10, 64)
    y3b, y1b = ops.conv3x3s2_pair_fwd(x, w10, 64)
    assert torch.equal(y3, y3b) and torch.equal(y1, y1b) and stats.shape[1] * cnt == 3 * (H // 2) ** 2
    _verify_train_pre("pair_stats H=%d mt=%s" % (H, mt), ops, y3, stats, cnt, w2, seed)


# ---- ee_syncbn_*: the local halves of SyncBatchNorm, for W simulated ranks in this one process ------------------------------------------
def _sync_ranks(ops, c, parts, res, two_addends=False, mask_from_x=False, want_dres=None):
    """The four ee_syncbn_* entry points in the order eeadv.syncbn.SyncBnActFn issues them, for every rank `parts` (index lists, a partition
    of the batch) deals images to, one rank after another on this device.  The all_gather is a stack of the ranks' moments in rank order,
    the all_reduce a sum of the ranks' sums in rank order; no process group, nothing spawned.  Returns whole-batch y / dx / dresidual, the
    statistics as rank 0 holds them (`ranks`: as every rank holds them), every rank's own [C, 2] sums (`local`) and their sum."""
    shard = lambda t: [t[idx].contiguous() for idx in parts]
    W = len(parts)
    xs, dys, d2s = shard(c["x"]), shard(c["dy"]), [None] * W
    rs = shard(c["residual"]) if res else [None] * W
    if two_addends:  # dy as two addends whose fp32 sum is exact: the kernels add them on load
        hi, lo = R.exact_addends(c["dy"])
        assert torch.equal(hi + lo, c["dy"]) and bool((lo != 0).any())
        dys, d2s = shard(hi), shard(lo)
    all_moments = torch.stack([ops.syncbn_stats(x) for x in xs])  # [W, C, 3]
    ranks = []
    for x, r in zip(xs, rs):
        rm, rv = c["rm"].clone(), c["rv"].clone()
        y, sm, si = ops.syncbn_apply(x, r, c["gamma"], c["beta"], all_moments, rm, rv, MOM, EPS, True)
        ranks.append({"y": y, "mean": sm, "invstd": si, "running_mean": rm, "running_var": rv})
    ys = [None if mask_from_x else f["y"] for f in ranks]
    local = [ops.syncbn_bwd_sums(dy, d2, y, x, c["gamma"], c["beta"], f["mean"], f["invstd"], True) for dy, d2, y, x, f in zip(dys, d2s, ys, xs, ranks)]
    total = local[0].clone()
    for s in local[1:]:
        total = total + s
    n_global = float(all_moments[:, 0, 2].sum().item())
    want_dres = res if want_dres is None else want_dres
    bw = [ops.syncbn_bwd_apply(dy, d2, y, x, c["gamma"], c["beta"], f["mean"], f["invstd"], total, n_global, True, True, want_dres)
          for dy, d2, y, x, f in zip(dys, d2s, ys, xs, ranks)]
    out = {k: ranks[0][k] for k in ("mean", "invstd", "running_mean", "running_var")}
    out.update(y=R.gather_back([f["y"] for f in ranks], parts), dx=R.gather_back([b[0] for b in bw], parts),
               dresidual=R.gather_back([b[1] for b in bw], parts) if want_dres else None, dgamma=total[:, 1].contiguous(), dbeta=total[:, 0].contiguous(),
               all_moments=all_moments, ranks=ranks, local=local)
    return out


SYNC_BITS = ("mean", "invstd", "running_mean", "running_var", "y", "dx", "dresidual", "dgamma", "dbeta", "all_moments")


def _sync_same_bits(case, a, b, what, keys=SYNC_BITS):
    for k in keys:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), "%s: %s %s" % (case, k, what)
    if "dgamma" in keys:
        for r, (u, v) in enumerate(zip(a["local"], b["local"])):
            assert torch.equal(u, v), "%s: rank %d's sums %s" % (case, r, what)


def _stock_rank_grads(c, res, parts):
    """torch's stock fp32 batch_norm / autograd over the whole batch with the incoming gradient zeroed outside one rank's images: that rank's
    share of (dgamma, dbeta) as the stock kernels sum it, [W, C] each - and the float64 shares on the stock ReLU branch"""
    w, b = (c[k].clone().requires_grad_(True) for k in ("gamma", "beta"))
    pre = F.batch_norm(c["x"], c["rm"].clone(), c["rv"].clone(), w, b, True, MOM, EPS)
    y = F.relu(pre + c["residual"] if res else pre)
    dg, db = [], []
    for idx in parts:
        dy_r = torch.zeros_like(c["dy"])
        dy_r[idx] = c["dy"][idx]
        g = torch.autograd.grad(y, [w, b], dy_r, retain_graph=True)
        dg.append(g[0])
        db.append(g[1])
    st = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, True, relu=True)
    ref_dg, ref_db = R.rank_param_grads64(c["x"], st["mean"], st["invstd"], c["dy"], y.detach() > 0, parts)
    return torch.stack(dg), torch.stack(db), ref_dg, ref_db


def _sync_verify(case, c, got, parts, res):
    """the whole batch against bn_ref64 (_verify: exact on `const` / gamma == 0 channels, bounded elsewhere, masks), then every rank's own
    sums against that rank's float64 share, the floor's n the rank's own element count"""
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, True, residual=c["residual"] if res else None, relu=True,
                     dy=c["dy"], mask=got["y"] > 0)
    _verify(case, c, got, ref, True, res, True, not res)
    ref_dg, ref_db = R.rank_param_grads64(c["x"], ref["mean"], ref["invstd"], c["dy"], got["y"] > 0, parts)
    stock_dg, stock_db, sref_dg, sref_db = _stock_rank_grads(c, res, parts)
    per_image = c["x"][0, 0].numel()
    for r, idx in enumerate(parts):
        who = "%s rank %d of %d" % (case, r, len(parts))
        _bounded(who, "dgamma", got["local"][r][:, 1], ref_dg[r], stock_dg[r], sref_dg[r], c["kinds"], len(idx) * per_image)
        _bounded(who, "dbeta", got["local"][r][:, 0], ref_db[r], stock_db[r], sref_db[r], c["kinds"], len(idx) * per_image)


SYNC_PATHS = [(name, label) for name in R.SYNC_CASES for label in R.SYNC_DEALS[name]]


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("name,label", SYNC_PATHS)
def test_syncbn_kernels_over_simulated_ranks(ops, name, label, res):
    shape, seed = R.SYNC_CASES[name]
    parts = R.SYNC_DEALS[name][label]
    c = _to_dev(R.hard_case(shape, seed))
    case = "syncbn %s %s%s" % (name, label, " +res" if res else "")
    assert all(ops.syncbn_supported(c["x"][idx].contiguous()) for idx in parts)
    got = _sync_ranks(ops, c, parts, res)
    _sync_same_bits(case, got, _sync_ranks(ops, c, parts, res), "differs between two runs")
    # every rank merges the same moments in the same order: the statistics are the same bits everywhere
    for r, f in enumerate(got["ranks"]):
        for k in ("mean", "invstd", "running_mean", "running_var"):
            assert torch.equal(f[k], got["ranks"][0][k]), "%s: rank %d's %s differs from rank 0's" % (case, r, k)
    # a rank's moments of a `const` channel are exactly (0.75, 0, its count); _verify then holds the merged statistics to _exact_stats
    const = [i for i, k in enumerate(c["kinds"]) if k == "const"]
    for r, idx in enumerate(parts):
        want = torch.tensor([R.CONST, 0.0, float(len(idx) * shape[2] * shape[3])], device=DEV)
        assert bool((got["all_moments"][r, const] == want).all()), "%s: rank %d's moments of the constant channels" % (case, r)
        assert bool((got["all_moments"][r, :, 2] == want[2]).all()), "%s: rank %d's counts" % (case, r)
    # the other forms of the backward return the bits of the plain one
    back = ("dx", "dresidual", "dgamma", "dbeta")
    if not res:
        _sync_same_bits(case, got, _sync_ranks(ops, c, parts, res, mask_from_x=True), "with the mask from x differs from the mask from y", back)
    _sync_same_bits(case, got, _sync_ranks(ops, c, parts, res, two_addends=True), "with dy in two addends differs", back)
    other = _sync_ranks(ops, c, parts, res, want_dres=not res)
    _sync_same_bits(case, got, other, "differs when dresidual is %s" % ("left out" if res else "asked for"), ("dx", "dgamma", "dbeta"))
    if not res:  # dresidual is dz itself
        assert torch.equal(other["dresidual"], torch.where(got["y"] > 0, c["dy"], torch.zeros_like(c["dy"]))), case + ": dresidual != dy under the mask"
    _sync_verify(case, c, got, parts, res)
    # the ranks in the opposite order (the merge and the sum of the sums run backwards): other bits, the same bounds
    _sync_verify(case + " reversed", c, _sync_ranks(ops, c, parts[::-1], res), parts[::-1], res)


def _sync_module(c):
    """a training-mode eeadv.syncbn.SyncBatchNorm2d (converted from models.BatchNorm2d, no process group) carrying the case's affine pair
    and running statistics"""
    from eeadv import models, syncbn
    bn = models.BatchNorm2d(len(c["kinds"]), eps=EPS, momentum=MOM)
    sbn = syncbn.convert_sync_batchnorm(torch.nn.Sequential(bn))[0].to(DEV).train()
    assert isinstance(sbn, syncbn.SyncBatchNorm2d)
    with torch.no_grad():
        for p, v in ((sbn.weight, c["gamma"]), (sbn.bias, c["beta"]), (sbn.running_mean, c["rm"]), (sbn.running_var, c["rv"])):
            p.copy_(v)
    return sbn


@pytest.mark.parametrize("equal_shards", [True, False])
@pytest.mark.parametrize("res", [False, True])
def test_syncbn_module_one_rank_on_hard_channels(ops, monkeypatch, res, equal_shards):
    """eeadv.syncbn.SyncBnActFn through models.bn_act on a converted SyncBatchNorm2d, no process group: the exchange is the identity, the
    global count host arithmetic (_EQUAL_SHARDS) or read from the moments"""
    from eeadv import models, syncbn
    shape, seed = R.SYNC_CASES["two-slices"]
    c = _to_dev(R.hard_case(shape, seed))
    monkeypatch.setattr(syncbn, "_EQUAL_SHARDS", equal_shards)
    seen = []
    apply = ops.syncbn_apply
    monkeypatch.setattr(syncbn.ops, "syncbn_apply", lambda *a: seen.append(apply(*a)) or seen[-1])
    sbn = _sync_module(c)
    x = c["x"].clone().requires_grad_(True)
    r = c["residual"].clone().requires_grad_(True) if res else None
    y = models.bn_act(sbn, x, r, relu=True)
    y.backward(c["dy"])
    assert len(seen) == 1, "the module did not take the ee_syncbn_* path"
    got = {"y": y.detach(), "mean": seen[0][1], "invstd": seen[0][2], "running_mean": sbn.running_mean, "running_var": sbn.running_var, "dx": x.grad,
           "dresidual": r.grad if res else None, "dgamma": sbn.weight.grad, "dbeta": sbn.bias.grad}
    ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, True, residual=c["residual"] if res else None, relu=True,
                     dy=c["dy"], mask=got["y"] > 0)
    _verify("syncbn module two-slices%s equal_shards=%s" % (" +res" if res else "", equal_shards), c, got, ref, True, res, True, not res)


@pytest.mark.parametrize("which", ["x", "residual"])
def test_syncbn_module_sends_a_misaligned_tensor_to_the_parent_path(ops, monkeypatch, which):
    """a dense view that starts one float into its storage: the ee_syncbn_* entry points refuse it (they read float4), so the module
    must not offer it to them - nn.SyncBatchNorm's own forward takes over, and the result is still that of bn_ref64"""
    from eeadv import _native as N, models, syncbn
    shape, seed = R.SYNC_CASES["one-slice"]
    c = _to_dev(R.hard_case(shape, seed))
    with pytest.raises(N.EEError, match="not aligned"):  # ee_syncbn_stats_f32 checks the pointer before its first launch
        ops.syncbn_stats(_misaligned(c["x"]))
    assert ops.syncbn_supported(c["x"]) and not ops.syncbn_supported(_misaligned(c["x"]))
    calls = []
    stats = ops.syncbn_stats
    monkeypatch.setattr(syncbn.ops, "syncbn_stats", lambda t: calls.append(1) or stats(t))
    for res in ((False, True) if which == "x" else (True,)):
        sbn = _sync_module(c)
        x = (_misaligned(c["x"]) if which == "x" else c["x"].clone()).requires_grad_(True)
        r = (_misaligned(c["residual"]) if which == "residual" else c["residual"].clone()).requires_grad_(True) if res else None
        assert sbn._fast(x) == (which != "x")
        y = models.bn_act(sbn, x, r, relu=True)
        y.backward(c["dy"])
        assert not calls, "a misaligned %s reached the ee_syncbn_* kernels" % which
        ref = R.bn_ref64(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, True, residual=c["residual"] if res else None, relu=True,
                         dy=c["dy"], mask=y.detach() > 0)
        case = "syncbn misaligned %s%s" % (which, " +res" if res else "")
        n = c["x"].numel() // shape[1]
        for name, t in (("y", y.detach()), ("dx", x.grad)):  # the floors alone: the reference stands in for the stock side, whose error is then 0
            _bounded(case, name, t, ref[name], ref[name], ref[name], c["kinds"], n)


def test_syncbn_module_copies_a_misaligned_incoming_gradient(ops, monkeypatch):
    """aligned x and residual take the ee_syncbn_* path; an incoming gradient that starts off a 16-byte boundary is copied, not refused"""
    from eeadv import models, syncbn
    shape, seed = R.SYNC_CASES["one-slice"]
    c = _to_dev(R.hard_case(shape, seed))
    calls, grads = [], []
    stats = ops.syncbn_stats
    monkeypatch.setattr(syncbn.ops, "syncbn_stats", lambda t: calls.append(1) or stats(t))
    for dy in (c["dy"], _misaligned(c["dy"])):
        sbn, x = _sync_module(c), c["x"].clone().requires_grad_(True)
        models.bn_act(sbn, x, c["residual"], relu=True).backward(dy)
        grads.append((x.grad, sbn.weight.grad, sbn.bias.grad))
    assert calls == [1, 1] and all(torch.equal(u, v) for u, v in zip(*grads))
