/*
 * uresnet_hip.h -- C-ABI of the MI355X-native U-ResNet forward/backward hot path.
 *
 * The reference (DeepLearnPhysics/u-resnet) has no FFI: the path sits behind a Python
 * class protocol (lib/ssnet.py ssnet_base) whose methods each issue one tf.Session.run
 * fetch-set.  This header declares one entry point per fetch-set plus lifecycle, so a
 * Python 3 `ssnet_base` (u-resnet_amd/ssnet.py) binds them with ctypes and keeps the
 * reference surface.  Citations are file:line relative to the reference tree.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; ursn_last_error() gives text;
 *   - all tensor pointers are DEVICE pointers (hipMalloc'd or torch tensor.data_ptr());
 *     the caller owns every buffer it passes in, the library owns only the host-side handle;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - layouts follow the reference: activations N(D)HWC row-major (lib/ssnet.py:34-40),
 *     conv filters [k..,Cin,Cout], transposed-conv filters [k..,Cout,Cin];
 *   - one handle per GPU; calls on a handle are serialised by the caller (the reference
 *     issues all sess.run calls from one thread, lib/ssnet_trainval.py:156-233).
 */
#ifndef URESNET_HIP_H
#define URESNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URSN_ABI_VERSION 9

typedef struct ursn_net ursn_net; /* opaque */

/* Mirrors uresnet.__init__ (lib/uresnet.py:15-20) + ssnet_base.construct (lib/ssnet.py:20-24). */
typedef struct ursn_config {
  int32_t ndim;          /* 2 (H,W,C) or 3 (H,W,D,C): len(dims)-1, lib/ssnet.py:11-14            */
  int32_t spatial[3];    /* dims[:-1]; spatial[2] unused for ndim==2; each divisible by 2^strides */
  int32_t cin;           /* dims[-1]                                                              */
  int32_t base_filters;  /* base_num_outputs, lib/uresnet.py:18                                   */
  int32_t num_class;     /* lib/ssnet.py:15                                                       */
  int32_t num_strides;   /* lib/uresnet.py:19 (reference fixes 5)                                 */
  int32_t max_batch;     /* largest N any call will pass (placeholder dim is None in the ref)     */
  int32_t trainable;     /* construct(trainable=...): allocate the backward workspace             */
  int32_t use_weight;    /* construct(use_weight=...), lib/ssnet.py:68-69                         */
  float bn_eps;          /* slim.batch_norm epsilon (default 1e-3)                                */
  int32_t act_dtype;     /* 0: fp32 everywhere (the reference's precision).  1: bf16 mixed precision
                          * (BASELINE.json configs[4]): activations, raw conv outputs and gradient tensors
                          * live in HBM as bf16, convolutions run on bf16 MFMA with fp32 accumulation;
                          * parameters, BatchNorm statistics, accumulated gradients and Adam stay fp32.
                          * Needs cin == 1 and base_filters % 8 == 0.                               */
} ursn_config;

typedef struct ursn_sizes {
  int64_t n_params;        /* trainable floats (weights + BN beta), TF variable order             */
  int64_t n_tensors;       /* number of trainable variables (2 per conv-like layer)               */
  int64_t n_layers;        /* conv-like layers (58 for num_strides=5)                             */
  int64_t workspace_bytes; /* device bytes for activations / stashes / scratch at max_batch       */
} ursn_sizes;

typedef struct ursn_param_info {
  char name[128];      /* TF variable name, e.g. "UResNet/conv0/weights"                          */
  int64_t offset;      /* float offset inside the flat parameter / gradient buffers              */
  int64_t nelem;
  int32_t rank;
  int32_t shape[5];
} ursn_param_info;

/* ---- lifecycle ------------------------------------------------------------------------ */
int ursn_abi_version(void);
const char* ursn_last_error(void);

/* Size query; no device access. */
int ursn_query(const ursn_config* cfg, ursn_sizes* out);

/* The plan a configuration compiles to, without device access: conv-like layer `index` in TF variable order
 * (lib/uresnet.py:37-121, lib/resnet_module.py:25-66) and the operand order of decoder step `step`'s tf.concat
 * (lib/uresnet.py:81: [deconv_i, skip]).  ssnet_base.construct checks what _build recorded against these. */
typedef struct ursn_layer_info {
  char name[96];       /* TF scope, e.g. "UResNet/resnet_module0/module1/shortcut"                 */
  int32_t transposed;  /* 0 slim.conv{2,3}d, 1 slim.conv{2,3}d_transpose                            */
  int32_t k, stride, cin, cout;
  int32_t relu;        /* activation_fn: 1 = tf.nn.relu (conv0, deconv*, conv1), 0 = None            */
  int64_t w_offset;    /* float offsets of `weights` and `BatchNorm/beta` in the flat buffers       */
  int64_t beta_offset;
} ursn_layer_info;
int ursn_query_layer(const ursn_config* cfg, int64_t index, ursn_layer_info* out);
int ursn_query_concat(const ursn_config* cfg, int32_t step, char* first, char* second, size_t cap);

/* Replaces graph construction (lib/ssnet.py:20-89 + lib/uresnet.py:22-123).  The four flat
 * fp32 buffers (n_params floats each) and the workspace are caller-owned device memory;
 * `grads` is the accum_vars set (lib/ssnet.py:53-55), adam_m/adam_v the Adam slots.
 * grads/adam_m/adam_v may be NULL when cfg->trainable == 0.
 *
 * Contract of the workspace and of the calls below (pinned by tests/test_state_independence_gpu.py):
 *   - the workspace needs NO initialisation: it may hold anything (zeros, NaNs, the remains of another plan) when it is
 *     handed over.  ursn_create clears the few regions no kernel writes and some kernel reads; every other byte a call reads
 *     was written earlier in the same call;
 *   - between ursn_create and ursn_destroy the workspace belongs to the handle: the caller neither writes it nor relies on
 *     its contents (ursn_tensor is a debug view of the LAST call);
 *   - a call's results depend only on its arguments, the parameter / gradient / Adam buffers and the Adam step counter: not
 *     on what the workspace held at create, not on the calls (kinds, batch sizes, inputs) the handle served before, and not
 *     on whether the host synchronised between enqueues.  Two such calls give the same BITS (no atomics, fixed-order
 *     reductions, streams ordered by events). */
int ursn_create(const ursn_config* cfg, float* params, float* grads, float* adam_m, float* adam_v,
                void* workspace, size_t workspace_bytes, ursn_net** out);
int ursn_destroy(ursn_net* net);
int ursn_get_sizes(const ursn_net* net, ursn_sizes* out);
int ursn_param(const ursn_net* net, int64_t index, ursn_param_info* out);

/* ---- the fetch-sets of lib/ssnet.py:91-139 --------------------------------------------- */
/* zero_gradients (lib/ssnet.py:99-101). */
int ursn_zero_grad(ursn_net* net, void* stream);

/* accum_gradients (lib/ssnet.py:103-115): forward + loss + backward, gradients ADDED into
 * `grads` (assign_add, :77).  data [N,prod(dims)], label/weight [N,prod(dims[:-1])] fp32 (label
 * values are class indices stored as float, :32,40).  weight may be NULL iff use_weight==0.
 * If out3 != NULL the call synchronises the stream and writes {loss, acc_all, acc_nonzero};
 * if NULL it only enqueues (metrics stay on the device, see ursn_read_metrics). */
int ursn_accum_step(ursn_net* net, const float* data, const float* label, const float* weight,
                    int32_t n, float* out3, void* stream);

/* apply_gradients (lib/ssnet.py:117-119): TF-form Adam on the accumulated gradients.
 * lr<=0 selects the TF default 1e-3 (lib/ssnet.py:72-75). The step counter is kept in the handle. */
int ursn_apply_adam(ursn_net* net, float lr, void* stream);

/* run_test (lib/ssnet.py:121-128): forward + {loss, acc_all, acc_nonzero}, no gradients. */
int ursn_eval(ursn_net* net, const float* data, const float* label, const float* weight, int32_t n,
              float* out3, void* stream);

/* inference (lib/ssnet.py:130-139): softmax_out [N,*spatial,num_class]; if label != NULL also
 * out2 = {acc_all, acc_nonzero}.  Always synchronises. */
int ursn_infer(ursn_net* net, const float* data, const float* label, int32_t n, float* softmax_out,
               float* out2, void* stream);

/* ana_step's label rule on the device (lib/ssnet_trainval.py:285-287): labels_out [N,*spatial] =
 * ((p[1] > p[2]) * 1 + (p[2] >= p[1]) * 2) * (data > 1.0), from the same forward pass as the optional softmax_out
 * (NULL: the softmax never leaves the kernel) and, if label != NULL, out2 = {acc_all, acc_nonzero}
 * (the reference prints acc_nonzero per entry, lib/ssnet_trainval.py:262).  Synchronises. */
int ursn_infer_labels(ursn_net* net, const float* data, const float* label, int32_t n, float* labels_out,
                      float* softmax_out, float* out2, void* stream);

/* Metrics of the last accum/eval call: synchronises, writes {loss, acc_all, acc_nonzero}. */
int ursn_read_metrics(ursn_net* net, float* out3, void* stream);

/* Adam step counter access (checkpoint / tests). */
int ursn_get_adam_step(const ursn_net* net, int64_t* t);
int ursn_set_adam_step(ursn_net* net, int64_t t);

/* Debug/parity: device pointer + channel stride of a named internal tensor of the last forward.
 * name = TF scope ("UResNet/conv0", ".../module1") optionally suffixed ":z" (raw conv output). */
int ursn_tensor(const ursn_net* net, const char* name, float** ptr, int64_t* voxels, int32_t* channels,
                int32_t* cstride);

/* Per-launch timing with HIP events recorded on the launch stream (bench.py roofline leg; the
 * reference has no counterpart: lib/ssnet_trainval.py:48-49 only reports peak bytes).
 * pass: 0 conv fwd, 1 conv dgrad, 2 conv wgrad, 3 bn stats, 4 bn apply, 5 bn backward, 6 head (the dense head records
 * kernel "head" / "bhead", the gather head of ursn_infer_voxels "vscores", the statistics of ursn_infer_stats "cstats"),
 * 7 BatchNorm moving statistics ("bn_moving_update", "bn_frozen_load": one launch for all layers). */
typedef struct ursn_prof_rec {
  char kernel[48];
  char layer[96];
  int32_t pass;
  float ms;
  double flops; /* algorithmic: 2*MACs of the layer */
  double bytes; /* algorithmic: x + y + w (fwd), dy + w + dx (dgrad), x + dy + dw (wgrad) */
  int32_t launches; /* launches of the named kernel inside this record (channel-block / split-input passes) */
  int32_t reserved_;
} ursn_prof_rec;
int ursn_profile_enable(ursn_net* net, int32_t on);
/* out == NULL: only counts.  Otherwise fills up to max_recs records and clears the log. */
int ursn_profile_read(ursn_net* net, ursn_prof_rec* out, int64_t max_recs, int64_t* n_out);

/* Weight gradients normally run on a second internal stream, overlapped with the data-gradient / BN-backward chain.
 * on = 0 serialises them on the caller's stream (per-kernel timing: concurrent kernels time-slice, so event intervals
 * would include the partner's work). */
int ursn_set_wgrad_overlap(ursn_net* net, int32_t on);
/* Name of the kernel the calling thread's last op-level / net-level dispatch chose (e.g. "tconv<8,8>", "bcbconv_bf16+pw"):
 * what ursn_prof_rec.kernel is filled from; the dispatch tests assert it.  Static storage, never NULL. */
const char* ursn_last_kernel_name(void);

/* ---- op-level entry points (unit parity tests; same kernels the net-level calls use) ----- */
typedef struct ursn_conv_desc {
  int32_t ndim;        /* 2 or 3                                                                   */
  int32_t n;           /* batch                                                                    */
  int32_t in_sp[3];    /* input spatial dims                                                       */
  int32_t cin, cout;
  int32_t k;           /* 1 or 3                                                                   */
  int32_t stride;      /* 1 or 2                                                                   */
  int32_t transposed;  /* 0: slim.conv{2,3}d SAME; 1: slim.conv{2,3}d_transpose k3 s2 SAME          */
  int32_t in_cstride;  /* channel stride (floats per voxel) of x / dx; 0 = compact (= cin)         */
  int32_t out_cstride; /* channel stride of y / dy; 0 = compact (= cout)                           */
  int32_t algo;        /* 0 auto, 1 naive reference, 2 gather MFMA, 3 tiled small-C, 4 LDS implicit GEMM, 5 pointwise, 6 LDS stride-2 gather, 7 LDS stride-2 scatter */
  /* Split input (a tf.concat that is never materialised, lib/uresnet.py:81): channels [0,in_split) of the layer input
   * live in x / dx, channels [in_split,cin) in x2 / dx2.  in_split = 0: single tensor.  Only k3 s1 and k1 s1 layers with
   * in_split = cin/2 on the tiled / pointwise kernels; other shapes return an error.                                   */
  int32_t in_split;
  int32_t in2_cstride; /* channel stride of x2 / dx2; 0 = compact (= cin - in_split)                                   */
  const float* x2;     /* forward and weight gradient: second input tensor                                            */
  float* dx2;          /* data gradient: second output tensor                                                         */
  /* Data gradient only: fused term of a parallel 1x1 conv with the same cin / cout and stride (the residual unit's shortcut,
   * lib/resnet_module.py:25-33): dx (+)= conv^T(dy, w) + pw_dy . pw_w^T.  pw_dy = NULL: none.  k3 s1 layers on the tiled /
   * all-taps kernels; fp32 k3 s2 layers 8 | 16 <- 16 channels on the lane-per-low-res-voxel kernel (the 1x1 stride-2 shortcut
   * touches the even-even-even voxels only; deconv_tiled_kernel.h).  Any other shape with pw_dy set is refused. */
  const float* pw_dy;  /* [voxels][cout] gradient at the shortcut conv's output                                       */
  const float* pw_w;   /* [cin][cout] shortcut weights                                                                 */
  int32_t pw_dy_cstride; /* 0 = compact (= cout)                                                                       */
  int32_t dtype;         /* 0: fp32 tensors.  1: x / y / dx / dy (and pw_dy, dx2) are bf16 (uint16 bit patterns), channel counts and
                          * strides multiples of 8, weights and dw stay fp32 (BASELINE configs[4] mixed precision).  The fused forms
                          * of the bf16 plan are reachable here on the shapes its dedicated kernels take (3-D k3 s1, 8 / 16 channels):
                          * in_mean / in_rstd / in_beta / in_relu (forward C -> C and weight gradient), pw_dy / pw_w (data gradient of a
                          * 16 -> 8 layer), in_split = 8 with dx2 (that data gradient written as two 8-channel tensors), and cin = 1:
                          * x is ONE fp32 channel per voxel (the network input read by conv0's forward and weight gradient)         */
  /* Normalise-on-load (forward and weight gradient): x is the RAW output z of the preceding conv whose BatchNorm has no
   * activation (resnet_conv1 inside a residual unit, lib/resnet_module.py:43-51); the kernel stages
   * (z - in_mean) * in_rstd + in_beta per input channel (zero padding stays zero), so that activation is never
   * written.  NULL: x is used as is.  k3 s1 tiled kernels with 8 / 16 input channels only.                          */
  const float* in_mean;
  const float* in_rstd;
  const float* in_beta;
  /* Data gradient only: the BatchNorm-backward reductions of the layer(s) whose INPUT gradient this call finishes, fused
   * into its epilogue (slim.batch_norm backward, lib/resnet_module.py:31,49,64: dz = r (g - mean g - xhat mean(g xhat))):
   * with g = dx * mask, bs_partial[block][0][c] = sum g, [1][c] = sum g * xhat(bs_z), [2][c] = sum g * xhat(bs_z2) over the
   * voxels of the block, ursn_conv_bs_blocks(d) blocks of 3 * cin doubles.  bs_relu: 0 no mask, 1 mask = bn(bs_z) > 0 (needs
   * bs_beta), 2 mask = the bit mask a residual join's forward wrote (bs_mask).  bs_z2 (optional): the second BatchNorm'd
   * branch of a residual join.  With a split input the reductions cover dx (the first tensor) only.
   * bs_partial = NULL: none.  3-D k3 s1 tiled kernels with 8 input channels per tensor only.                              */
  const float* bs_z;
  const float* bs_mean;
  const float* bs_rstd;
  const float* bs_beta;
  const float* bs_z2;
  const float* bs_mean2;
  const float* bs_rstd2;
  const void* bs_mask;
  double* bs_partial;
  int32_t bs_z_cstride;  /* 0 = compact */
  int32_t bs_z2_cstride;
  int32_t bs_relu;
  int32_t in_relu;       /* normalise-on-load with the producer's ReLU: stages max(bn(z), 0) (dtype 1 only: conv1 -> conv2,
                          * lib/uresnet.py:103-121)                                                                              */
  /* Data gradient only (ABI 7): BatchNorm-backward APPLY on load (slim.batch_norm backward of THIS layer, lib/resnet_module.py:49,
   * lib/uresnet.py:109).  The `dy` argument of ursn_conv_backward_data is then g, the gradient at the BatchNorm's OUTPUT, and
   * the kernel forms, per channel c, while it stages its operand
   *     dz = A g' + B (z - mu) + C,    g' = g * (fma(z, S, T) > 0)  if vdz_relu  else g
   * with vdz_coef = [6][cout] floats {A, B, C, mu, S, T} (A = S = rstd, B = -rstd^2 mean(g' xhat), C = -rstd mean(g'),
   * T = beta - mu rstd: what ursn_net's BatchNorm-backward finalise writes), uses it for dx and STORES it to vdz_out (same
   * layout / channel stride as dy): the weight gradient reads dz there and the separate apply pass (read g, z; write dz)
   * disappears.  3-D k3 s1 layers with cin = cout = 8 on the tiled kernels; z, dy and vdz_out share out_cstride.  NULL: off. */
  const float* vdz_z;
  const float* vdz_coef;
  float* vdz_out;
  int32_t vdz_relu;
} ursn_conv_desc;

/* y = conv(x, w).  w layout [k..,Cin,Cout] (transposed: [k..,Cout,Cin]). */
int ursn_conv_forward(const ursn_conv_desc* d, const float* x, const float* w, float* y, void* stream);
/* y = conv(x, w) plus the batch statistics BatchNorm needs: mean[cout], rstd[cout] = rsqrt(var+eps)
 * (slim.batch_norm as normalizer_fn, lib/uresnet.py:42).  scratch: 8-byte aligned device buffer of at least
 * ursn_conv_stats_scratch_bytes(d) bytes (declared at the end of this header) -- the per-workgroup partial sums of the kernel
 * family this descriptor dispatches to, NOT a function of the voxel count alone; a smaller buffer is refused before any launch
 * ("scratch too small").  The scratch needs no initialisation. */
int ursn_conv_forward_stats(const ursn_conv_desc* d, const float* x, const float* w, float* y, float* mean,
                            float* rstd, float eps, void* scratch, size_t scratch_bytes, void* stream);
/* dx (=|+=) conv^T(dy, w); accumulate != 0 adds into dx. */
int ursn_conv_backward_data(const ursn_conv_desc* d, const float* dy, const float* w, float* dx,
                            int32_t accumulate, void* stream);
/* dw += x (*) dy.  scratch: device buffer of ursn_conv_wgrad_scratch_bytes(d) bytes. */
int ursn_conv_backward_weight(const ursn_conv_desc* d, const float* x, const float* dy, float* dw,
                              void* scratch, size_t scratch_bytes, void* stream);
size_t ursn_conv_wgrad_scratch_bytes(const ursn_conv_desc* d);
/* Blocks of bs_partial a data-gradient call with fused BatchNorm-backward reductions writes (0: shape not supported). */
int32_t ursn_conv_bs_blocks(const ursn_conv_desc* d);

/* "Explain plan": name of the kernel family the dispatcher hands this descriptor to (pass: 0 forward, 1 data gradient,
 * 2 weight gradient), e.g. "tconv", "igemm", "bdconv", "gconv_mfma".  Host logic only -- no device access, nothing runs:
 * what the plan-guard tests and tools/ query. */
int ursn_conv_plan(const ursn_conv_desc* d, int32_t pass, char* out, size_t cap);

/* Batch-statistics BatchNorm (beta only) + optional residual + optional ReLU:
 * y = act((z-mu)*rsqrt(var+eps)+beta [+ res]); stats_out (optional) gets {mean[C], rstd[C]} as fp32. */
int ursn_bn_forward(const float* z, const float* beta, const float* res, float* y, int64_t voxels,
                    int32_t channels, float eps, int32_t relu, float* stats_out, void* scratch,
                    size_t scratch_bytes, void* stream);
/* dz = BN backward of g = dy * (relu ? y>0 : 1); dbeta += sum g. */
int ursn_bn_backward(const float* dy, const float* y, const float* z, float* dz, float* dbeta,
                     int64_t voxels, int32_t channels, float eps, int32_t relu, void* scratch,
                     size_t scratch_bytes, void* stream);
size_t ursn_bn_scratch_bytes(int64_t voxels, int32_t channels);

/* BatchNorm passes of the bf16 plan at op level (slim.batch_norm forward / backward at lib/resnet_module.py:31,49,64 and
 * lib/uresnet.py:42,75,85,109,119 on bf16 tensors; bf16_elementwise.hip) with every optional operand the plan uses.  Tensors
 * are bf16 bit patterns with channel counts / strides multiples of 8; statistics, beta and d(beta) are fp32.
 *   forward : y = act(bn(z) [+ bn2(z2) | + res]); mask_out (relu): one byte per 16-byte piece of y, bit j = (channel j > 0);
 *             cat != 0 (8 channels): y[v] = [act(bn(z)) | act(bn2(z2))], both halves of a concat voxel in one store
 *   backward: g = (dy [+ dy2]) * mask, mask = the bytes `mask` | y > 0 | bn(z) > 0 (first that is given; relu != 0);
 *             dz = r (g - mean g - xhat mean(g xhat)), d(beta) += sum g; with z2: the join's second BatchNorm gets dz2 /
 *             dbeta2 from the same g; dres (=|+=) g is the identity shortcut's share (lib/resnet_module.py:22-23,68)     */
typedef struct ursn_bn_bf16_desc {
  int64_t voxels;
  int32_t channels, relu;
  const void* z;   int32_t z_cstride;   const float *mean, *rstd, *beta;
  const void* z2;  int32_t z2_cstride;  const float *mean2, *rstd2, *beta2;
  const void* res; int32_t res_cstride;
  void* y;         int32_t y_cstride;   /* forward output; backward: optional mask source (y > 0) */
  uint8_t* mask_out;
  int32_t cat;
  const void* dy;  int32_t dy_cstride;
  const void* dy2; int32_t dy2_cstride;
  const uint8_t* mask;
  void* dz;        int32_t dz_cstride;
  void* dz2;       int32_t dz2_cstride;
  float *dbeta, *dbeta2;
  void* dres;      int32_t dres_cstride; int32_t dres_accumulate;
} ursn_bn_bf16_desc;
int ursn_bn_bf16_forward(const ursn_bn_bf16_desc* d, void* stream);
int ursn_bn_bf16_backward(const ursn_bn_bf16_desc* d, void* scratch, size_t scratch_bytes, void* stream);
size_t ursn_bn_bf16_scratch_bytes(int64_t voxels, int32_t channels);

/* Fused head (lib/ssnet.py:57-71): softmax / weighted CE / accuracies / dlogits.
 * logits [n*pix, ncls]; data [n*pix] (cin==1); out3 = {loss, acc_all, acc_nonzero};
 * softmax_out, dlogits may be NULL. Synchronises. */
int ursn_softmax_ce(const float* logits, const float* data, const float* label, const float* weight,
                    int32_t n, int64_t pix, int32_t ncls, float* softmax_out, float* dlogits,
                    float* out3, void* scratch, size_t scratch_bytes, void* stream);

/* TF-form Adam on a flat buffer: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps). */
int ursn_adam(float* p, const float* g, float* m, float* v, int64_t nelem, float lr, float b1, float b2,
              float eps, int64_t t, void* stream);

/* ---- voxel-list I/O (ABI 8; voxel_io.hip) -------------------------------------------------------------------------
 * LArTPC events are almost empty and larcv hands them over as voxel lists; the reference also WRITES its 3-D ana product as a
 * voxel set (lib/ssnet_trainval.py:299-302: larcv.as_tensor3d(ssnet_result) into a sparse3d product).  The network stays
 * dense: these two stateless passes sit at its boundary.  Like the calls above, their results depend only on their arguments
 * (no atomics, fixed-order scans; the scratch buffer needs no initialisation). */
typedef struct ursn_voxel_batch {   /* all pointers are DEVICE pointers */
  int32_t n;                 /* events */
  int64_t voxels;            /* prod(spatial) of one event; cin == 1 */
  const int64_t* offsets;    /* [n+1], offsets[0] = 0: event i owns list entries [offsets[i], offsets[i+1]) */
  const int32_t* index;      /* [M] row-major voxel index inside the event, strictly increasing per event */
  const float* value;        /* [M] data */
  const float* label;        /* [M] class index as float (lib/ssnet.py:32,40) */
  const float* weight;       /* [M], NULL iff the dense weight output is NULL */
  const float* bg_weight;    /* [n] weight of every voxel NOT listed (inverse-frequency weights are non-zero on background) */
} ursn_voxel_batch;

/* dense data/label/weight [n, voxels] fp32 = background (0, 0, bg_weight[i]) overwritten at the listed voxels: the tensors
 * ursn_accum_step / ursn_eval / ursn_infer_labels read (lib/ssnet.py:141-153 feed_dict).  A fill pass (16-byte stores over every
 * byte of the outputs) and a scatter pass (an index outside [0, voxels) is skipped, never written) on `stream`.
 * Enqueues only; never synchronises.  label / weight may be NULL (inference feed). */
int ursn_voxels_to_dense(const ursn_voxel_batch* b, float* data, float* label, float* weight, void* stream);

/* Voxel set of a dense label volume (what larcv.as_tensor3d keeps, lib/ssnet_trainval.py:299-302): for each event, the voxels
 * with labels != 0 in increasing index order.  offsets_out [n+1] (device); index_out / class_out hold at most `cap` entries --
 * entries whose position is >= cap are not written, offsets_out still holds the true counts so the caller can see the overflow.
 * Three launches (per-block counts, one-workgroup exclusive scan, write); scratch >= ursn_labels_to_voxels_scratch_bytes(n, voxels).
 * Enqueues only. */
int ursn_labels_to_voxels(const float* labels, int32_t n, int64_t voxels, int32_t* index_out, uint8_t* class_out,
                          int64_t cap, int64_t* offsets_out, void* scratch, size_t scratch_bytes, void* stream);
size_t ursn_labels_to_voxels_scratch_bytes(int32_t n, int64_t voxels);

/* ---- voxel-list scores (ABI 9; voxel_io.hip) -----------------------------------------------------------------------
 * The output side of the voxel-list boundary: the reference's consumers read the softmax at an event's own voxels
 * (example_scripts/ana_csv.py per-class score means, the score renormalisation at lib/ssnet_trainval.py:280-283), so the class
 * scores, the argmax class and the ana label are gathered AT THE LISTED VOXELS from the stored raw logits of conv2 and the dense
 * [N, *spatial, num_class] softmax is never written.  For list entry m of event i, p = i * voxels + index[m]:
 *     logit[k] = fma(z[p][k], rstd[k], beta[k] - mean[k] * rstd[k]),  e[k] = exp(logit[k] - max),  score[k] = e[k] * (1 / sum e)
 * -- the arithmetic of the dense head of the same plan, in the same order (expf on fp32 logits, elementwise.hip; the fast
 * __expf on bf16 logits, bf16_elementwise.hip), so the scores carry the BITS of ursn_infer's softmax at those voxels. */
typedef struct ursn_vscores_desc {
  int32_t n; int64_t voxels; int32_t ncls;           /* events, prod(spatial) of one event, 1..8 classes              */
  const void* z; int32_t z_cstride; int32_t dtype;   /* 0 fp32 (stride >= ncls; 4 with <= 4 classes and a 16-byte aligned z: one
                                                      * 16-byte load), 1 bf16 bit patterns (stride 8, 16-byte aligned)    */
  const float *mean, *rstd, *beta;                   /* NULL mean: z already holds logits */
  const float* data;                                 /* [n, voxels], needed iff ana_out */
  const int64_t* offsets; const int32_t* index;      /* as in ursn_voxel_batch */
} ursn_vscores_desc;

/* scores_out [M, ncls] fp32, pred_out [M] uint8 (argmax, lowest index on ties), ana_out [M] uint8
 * (((p1 > p2) * 1 + (p2 >= p1) * 2) * (data[p] > 1.0), lib/ssnet_trainval.py:285-287; needs ncls >= 3); M = offsets[n].  Each
 * output may be NULL, not all three.  An entry whose index lies outside [0, voxels) reads nothing and gets zeros in every
 * requested row; events without entries are legal.  One launch of one thread per entry (the list length lives on the device,
 * so the grid is sized from `voxels` like the scatter pass of ursn_voxels_to_dense); no atomics, no scratch: the result depends
 * only on the arguments.  Enqueues only; never synchronises. */
int ursn_scores_at_voxels(const ursn_vscores_desc* d, float* scores_out, uint8_t* pred_out, uint8_t* ana_out, void* stream);

/* Forward pass, then the gather head on conv2's stored z / mean / rstd for the voxel list (offsets [n+1], index [m_total], device
 * pointers, as in ursn_voxel_batch; rows at or beyond m_total are never written, m_total = 0 launches no gather).  Outputs as in
 * ursn_scores_at_voxels.  label != NULL and out2 != NULL: the dense head also runs, without a softmax output, for out2 =
 * {acc_all, acc_nonzero} exactly as ursn_infer_labels gives them; label == NULL: the dense head is not launched at all.
 * Needs cin == 1 (ana_out: >= 3 classes).  Both plans.  Always synchronises, like ursn_infer. */
int ursn_infer_voxels(ursn_net* net, const float* data, const float* label, int32_t n, const int64_t* offsets,
                      const int32_t* index, int64_t m_total, float* scores_out, uint8_t* pred_out, uint8_t* ana_out,
                      float* out2, void* stream);

/* ---- per-event weight normalisation (weight_norm.hip) ----------------------------------------------------------------
 * Appended functions only: no existing declaration or struct layout changes, so URSN_ABI_VERSION stays 9. */

/* Per-event weight normalisation (lib/ssnet_trainval.py:173,204): out[e][v] = weight[e][v] / (float)S_e,
 * S_e = sum_v weight[e][v] in fp64, fixed order.  out may equal weight (in place).  sums_out [n] optional (device).
 * Two launches, no atomics, the scratch needs no initialisation; enqueues only, never synchronises.
 * The division is the IEEE correctly rounded fp32 one and nothing is special-cased: an event whose weights sum to zero gets
 * what numpy gives it (0/0 = NaN, x/0 = inf).  scratch: 8-byte aligned, >= ursn_normalize_weights_scratch_bytes(n, voxels)
 * (0 for n outside [1, 65535] or voxels outside [1, 2^31)); out must not overlap weight unless it equals it. */
int ursn_normalize_weights(const float* weight, float* out, int32_t n, int64_t voxels, float* sums_out,
                           void* scratch, size_t scratch_bytes, void* stream);
size_t ursn_normalize_weights_scratch_bytes(int32_t n, int64_t voxels);

/* ---- per-event, per-class analysis statistics (ana_stats.hip) --------------------------------------------------------
 * Appended functions and one struct only: URSN_ABI_VERSION stays 9.
 * What example_scripts/ana_csv.py:67-116 computes per event on the host from the dense softmax, reduced on the device from conv2's
 * stored logits: for voxel p of event e the logits, the prediction (strict '>' argmax, lowest index on ties: tf.argmax) and the
 * scores are formed exactly as ursn_scores_at_voxels forms them (same layouts, same bits), t = (int)label[p] truncates toward
 * zero like the dense head, and
 *   t in [0, C):  conf[e][t][pred] += 1, score_sum[e][t] += (double)score[t], score_sq[e][t] += (double)score[t] * score[t]
 *   otherwise  :  other[e][label > 0 ? 0 : 1] += 1 (a NaN label lands in other[e][1]); the voxel matches no prediction
 *   nonzero[e] = {voxels with data > 0, of those pred == t} (lib/ssnet.py:59; one input channel). */
typedef struct ursn_class_stats_out {      /* all DEVICE pointers, 8-byte aligned; each may be NULL except conf */
  int64_t* conf;      /* [n][C][C]  conf[e][t][p] = voxels of event e with label t and prediction p                */
  int64_t* other;     /* [n][2]     labels outside [0,C): {those > 0, the rest (<= 0 after the cast, NaN)}          */
  int64_t* nonzero;   /* [n][2]     {voxels with data > 0, of those pred == label}; needs d->data                  */
  double*  score_sum; /* [n][C]     sum over voxels with label k of score[k]                                       */
  double*  score_sq;  /* [n][C]     sum over the same voxels of score[k]^2                                         */
} ursn_class_stats_out;

/* d: n, voxels, ncls, z / z_cstride / dtype, mean / rstd / beta and data as in ursn_scores_at_voxels; offsets / index are unused and
 * may be NULL.  label [n, voxels] fp32.  Two launches: a workgroup owns a fixed compile-time span of 4096 consecutive voxels of one
 * event and writes its partial counts and fp64 sums to the scratch; a second launch reduces each event's partials in a fixed
 * tree.  No global atomics, the scratch needs no initialisation, the same arguments give the same bits; integer counts are
 * exact.  An event with no voxel of class k leaves zeros in row k.  Enqueues only; never synchronises.
 * scratch: 8-byte aligned, >= ursn_class_stats_scratch_bytes(n, voxels, ncls) (0 for n outside [1, 65535], voxels outside
 * [1, 2^31) or ncls outside [1, 8]).  Null, misaligned, out-of-domain and too-small arguments are refused before any launch. */
int ursn_class_stats(const ursn_vscores_desc* d, const float* label, const ursn_class_stats_out* out, void* scratch,
                     size_t scratch_bytes, void* stream);
size_t ursn_class_stats_scratch_bytes(int32_t n, int64_t voxels, int32_t ncls);

/* ursn_infer_labels with every dense output optional, plus the statistics: one forward pass, then ursn_class_stats on conv2's
 * stored z / mean / rstd (both plans) with scratch from the handle's workspace.  label and stats (stats->conf) are required.  The
 * dense head is launched only if one of labels_out / softmax_out / out2 is given and then writes exactly what ursn_infer_labels
 * writes (labels_out: >= 3 classes and cin == 1).  The statistics work for any num_class in 1..8 and any cin; with cin != 1
 * stats->nonzero must be NULL.  Recorded as pass 6, kernel "cstats", when profiling.  Always synchronises, like ursn_infer. */
int ursn_infer_stats(ursn_net* net, const float* data, const float* label, int32_t n, float* labels_out, float* softmax_out,
                     float* out2, const ursn_class_stats_out* stats, void* stream);

/* ---- external loss boundary (ext_loss.hip) ---------------------------------------------------------------------------
 * Appended functions only: URSN_ABI_VERSION stays 9.
 * The reference computes one loss, the weighted softmax cross-entropy of lib/ssnet.py:57-71, inside its graph.  These calls cut
 * the step open at the logits so that a caller's own objective (focal / dice terms, a masked or auxiliary loss, a distillation
 * target) can sit between the forward and the backward pass: logits out, d(loss)/d(logits) in, gradients ADDED to the flat
 * buffer exactly like ursn_accum_step's, and optionally d(loss)/d(input).  Every call below enqueues only and never
 * synchronises (on the bf16 plan the forward pass uploads its weight-packing table once per batch size, as in every other call);
 * null, misaligned, out-of-domain and too-small arguments are refused with a message before any launch. */

/* Dense logits from conv2's stored operands: logits_out [n, voxels, ncls] fp32, compact and channel-last,
 *     logit[k] = fma(z[p][k], rstd[k], beta[k] - mean[k] * rstd[k])
 * exactly as the heads and ursn_scores_at_voxels form it.  d: n, voxels, ncls, z / z_cstride / dtype, mean / rstd / beta as in
 * ursn_scores_at_voxels (fp32 at any stride >= ncls, one 16-byte load per voxel at stride 4 | 8 with a 16-byte aligned z; bf16 bit
 * patterns at stride 8; mean == NULL: z already holds logits); data / offsets / index are unused.  logits_out needs 4-byte
 * alignment only.  One launch, no atomics, no scratch. */
int ursn_logits_dense(const ursn_vscores_desc* d, float* logits_out, void* stream);

/* The caller's compact fp32 dlogits [n, voxels, ncls] in the layout of a plan's d(loss)/d(logits) tensor, written as the head of
 * that layout writes it: dtype 0, out_cstride 4 with <= 4 classes and a 16-byte aligned out: one 16-byte store per voxel, pad
 * lanes zero; dtype 0 otherwise (out_cstride >= ncls): the ncls values, pad lanes NOT written; dtype 1 (out_cstride 8, 16-byte
 * aligned): bf16 round-to-nearest-even, pad lanes zero.  One launch, no atomics, no scratch. */
int ursn_dlogits_pack(const float* dlogits, int32_t n, int64_t voxels, int32_t ncls, void* out, int32_t out_cstride,
                      int32_t dtype, void* stream);

/* Input gradient of the first convolution (k3 s1 SAME, lib/uresnet.py:37-45), which no step forms:
 *     dinput_out[n, p, c] = sum over the 3^ndim taps k and f < F of dz[n, p - (k - 1), f] * w[k, c, f]     (fp32, [n, voxels, cin])
 * dz: conv0's stored BatchNorm-backward output, fp32 at dz_cstride >= F floats (dtype 0) or bf16 bit patterns at a stride that
 * is a multiple of 8 (dtype 1: cin == 1, F % 8 == 0, 16-byte aligned).  w: the fp32 master weights [3^ndim, cin, F] as
 * ursn_param lays conv0's out; with dtype 1 they are rounded to bf16 on load, the value the bf16 plan's other data gradients
 * use.  fp32 accumulation.  One launch: the dz tile and its halo are staged once in LDS. */
int ursn_conv0_input_grad(int32_t ndim, const int32_t* spatial, int32_t n, int32_t cin, int32_t F, const void* dz,
                          int32_t dz_cstride, int32_t dtype, const float* w, float* dinput_out, void* stream);

/* The forward pass of ursn_accum_step (every stored operand is bit for bit what a step stores), then ursn_logits_dense on conv2's
 * operands; the head is not launched and the metrics buffer is not touched.  Needs a trainable handle.  logits_out
 * [n, *spatial, num_class] fp32.  Both plans.  Recorded as pass 6, kernel "logits", when profiling. */
int ursn_forward_logits(ursn_net* net, const float* data, int32_t n, float* logits_out, void* stream);

/* The backward pass of ursn_accum_step started from the caller's dlogits [n, *spatial, num_class] fp32: ursn_dlogits_pack into
 * the handle's d(logits) tensor -- with the BatchNorm-backward partials of the logits layer where the plan's head would have
 * carried them, in the head's partition and order, so that dlogits equal to the head's give the step's gradients bit for bit --
 * then the unchanged backward chain; gradients are ADDED to the flat buffer.  dinput_out (nullable) [n, *spatial, cin] fp32:
 * ursn_conv0_input_grad after conv0's BatchNorm backward has stored its dz.
 * Legal only directly after ursn_forward_logits on the same handle with the same n and data pointer: any run call in between
 * (accum_step, eval, every infer, another forward_logits), ursn_apply_adam, or a backward_logits that already consumed the
 * forward makes the call fail with a message naming the reason, before anything is launched.
 * Recorded as pass 6 "dlogits" and pass 1 "dinput" (layer conv0) when profiling. */
int ursn_backward_logits(ursn_net* net, const float* data, const float* dlogits, int32_t n, float* dinput_out, void* stream);

/* ---- cube-symmetry augmentation and test-time averaging (symmetry.hip) --------------------------------------------------
 * Appended functions and one struct only: URSN_ABI_VERSION stays 9.
 * What users of a 3-D segmentation trainer do on the host before the feed -- flip and transpose the (data, label, weight)
 * volumes -- and, on the analysis side, map the score volumes of several symmetric views back before averaging them.  An
 * operation is a small integer code; for one event x of shape [*spatial, C] it means
 *     out = np.flip(np.transpose(x, P[code >> ndim] + (ndim,)), axis=[a for a in range(ndim) if (code >> a) & 1])
 * with P the axis permutations in lexicographic order (3-D: (0,1,2),(0,2,1),(1,0,2),(1,2,0),(2,0,1),(2,1,0); 2-D: (0,1),(1,0)):
 * 48 codes in 3-D, 8 in 2-D, code 0 the identity, bit a flips OUTPUT axis a.  Equivalently input voxel i lands at output voxel o
 * with o[a] = f_a(i[P[a]]), f_a(t) = spatial[a] - 1 - t if bit a is set, else t.  A code is valid for a shape iff
 * spatial[P[a]] == spatial[a] for every a (the output then has the input's shape); any other code is refused.
 * The passes are pure data movement: output bits equal input bits (NaN payloads, -0.0).  Every call below enqueues only and
 * never synchronises, uses no atomics and no scratch, and its results depend only on its arguments; null, misaligned,
 * overlapping, out-of-domain or invalid-code arguments are refused with a message before anything is launched.  The codes are a
 * HOST array, validated on the host, and travel to the kernel as launch arguments (one byte per event: no H2D copy), which is
 * why these calls take n <= 1024. */
typedef struct ursn_sym_desc {
  int32_t ndim, spatial[3], n, channels;  /* ndim 2 | 3 (spatial[2] unused in 2-D); channels 1..8, channel-last;
                                           * prod(spatial) * channels < 2^31 */
  const int32_t* ops;                     /* HOST array, one code per event */
} ursn_sym_desc;

/* Host helpers, no device access: the number of codes (0 for ndim outside {2, 3}); whether `code` is valid for the shape (0 | 1);
 * the inverse code; the code of "b after a" (apply a, then b).  inverse / compose return -1 for a code outside [0, count). */
int ursn_sym_count(int32_t ndim);
int ursn_sym_valid(int32_t ndim, const int32_t* spatial, int32_t code);
int ursn_sym_inverse(int32_t ndim, int32_t code);
int ursn_sym_compose(int32_t ndim, int32_t a, int32_t b);

/* Up to three tensors [n, *spatial, channels] fp32 (the data / label / weight triple) permuted in ONE launch:
 * dst_k[e] = op[e](src_k[e]).  Later pairs may be NULL (a pair is either both set or both NULL); no dst may overlap any src or
 * another dst.  Pointers need 4-byte alignment only.  Events whose op keeps the last axis last copy whole rows (reversed when
 * flipped, 16-byte accesses where both sides are 16-byte aligned); events whose op moves the last axis transpose 32 x 32 tiles
 * through padded LDS, so that global reads and writes are both contiguous along the fastest axis of their tensor. */
int ursn_sym_apply(const ursn_sym_desc* d, const float* src0, float* dst0, const float* src1, float* dst1, const float* src2,
                   float* dst2, void* stream);

/* dst = ((first ? 0 : dst) + op(src)) * scale, one fp32 add then one fp32 multiply, same access pattern as ursn_sym_apply: the
 * back-mapping step of test-time averaging (the caller passes the INVERSE codes of the views).  first != 0: dst is not read. */
int ursn_sym_accumulate(const ursn_sym_desc* d, const float* src, float* dst, int32_t first, float scale, void* stream);

/* ursn_voxels_to_dense with the scatter writing list entry i at its image o under ops[event] (a bijection of the event's voxels, so
 * no two entries share an address; an index outside [0, voxels) is skipped).  The fill pass is ursn_voxels_to_dense's.
 * prod(spatial) must equal b->voxels; ops is a HOST array of b->n <= 1024 codes. */
int ursn_voxels_to_dense_sym(const ursn_voxel_batch* b, int32_t ndim, const int32_t* spatial, const int32_t* ops, float* data,
                             float* label, float* weight, void* stream);

/* The gather side: index_out[m] = image of index[m] under ops[event] for the entries [offsets[e], offsets[e+1]) of event e
 * (offsets [n+1], index / index_out [M]: device pointers; index_out may not overlap index).  An index outside [0, prod(spatial))
 * is copied unchanged.  The list that comes out is NOT sorted: it is in the order of `index`, entry m still belongs to the voxel
 * entry m came in as.  ursn_scores_at_voxels and ursn_infer_voxels need distinct indices per event only, not sorted ones, so
 * scores gathered on a transformed volume at index_out line up with the original list. */
int ursn_voxel_index_sym(int32_t ndim, const int32_t* spatial, int32_t n, const int32_t* ops, const int64_t* offsets,
                         const int32_t* index, int32_t* index_out, void* stream);

/* ---- BatchNorm moving statistics (bn_moving.hip) -------------------------------------------------------------------------
 * Appended functions only: URSN_ABI_VERSION stays 9.
 * The part of slim.batch_norm the reference leaves dead (is_training is never False and UPDATE_OPS never run): per BatchNorm layer
 * moving_mean[C] (initial 0) and moving_variance[C] (initial 1) in fp32, maintained by assign_moving_average without zero-debias,
 *     m <- m - momentum * (m - x),    momentum = 1 - decay (slim default decay 0.999),
 * x = the layer's batch mean, respectively its BIASED batch variance v = max(1 / (rstd * rstd) - eps, 0) recovered in fp64 from the
 * fp32 rstd the forward stores.  The whole update is fp64 with every operation rounded on its own (no FMA contraction) and rounded
 * to fp32 once: np.float32(m - mu * (m - x)) on float64 operands gives the same bits.
 * The moving buffer is caller-owned like `params`: 2 * sum(cout) floats, layer by layer in ursn_query_layer order, each layer
 * [moving_mean[cout] | moving_variance[cout]], unpadded.  It is not part of the workspace. */

/* Floats of the moving buffer of a configuration (2 * sum of cout over ursn_query_layer); no device access. */
int ursn_bn_moving_size(const ursn_config* cfg, int64_t* out);

/* Attaches the caller's buffer (NULL detaches; detaching while frozen is refused).  Nothing is launched, the buffer is not read. */
int ursn_bn_attach(ursn_net* net, float* moving);

/* Folds the batch statistics of the handle's LAST forward (any run call, both plans) into the attached buffer: ONE launch for all
 * layers on `stream`, enqueued only.  The forward joins its side stream before it returns, so a launch on the stream the run call
 * used is ordered after every writer of a layer's mean / rstd and before the next forward overwrites them.  Refused when no buffer
 * is attached, no forward has run, the last forward was frozen, or momentum lies outside [0, 1]. */
int ursn_bn_update(ursn_net* net, double momentum, void* stream);

/* The same kernel on flat contiguous vectors of `count` channels (mean / rstd in, moving_mean / moving_variance updated in place),
 * for tests and callers without a handle.  Null or misaligned pointers, count outside [1, 2^31), momentum outside [0, 1] and
 * eps <= 0 are refused before any device access.  One launch, enqueued only. */
int ursn_bn_moving_update(const float* mean, const float* rstd, float* moving_mean, float* moving_variance, int64_t count,
                          double momentum, float eps, void* stream);

/* on != 0: every forward-only entry (ursn_infer, ursn_infer_labels, ursn_infer_voxels, ursn_infer_stats, ursn_eval) normalises
 * every layer with the moving statistics, y = (z - moving_mean) * (1 / sqrt(moving_variance + eps)) + beta with the reciprocal
 * root formed like the kernels' own finalise forms rstd (fp64, rounded to fp32): ONE launch at the start of the call writes every
 * layer's mean / rstd vectors (pad lanes 0) from the buffer, and the conv kernels' statistics finalise is pointed at a scratch pair
 * nobody reads, so every consumer (BatchNorm passes, normalise-on-load, the heads, ursn_tensor's :mean / :rstd) sees the moving
 * values.  The statistics reductions inside the conv kernels still run.  While frozen, ursn_accum_step, ursn_forward_logits and
 * ursn_backward_logits are refused (frozen mode is forward-only).  Needs an attached buffer.  With nothing attached and frozen off
 * no call launches anything new or passes a different pointer.
 * When profiling, the load and ursn_bn_update's launch are recorded under a pass id of their own, 7, as kernels "bn_frozen_load" and
 * "bn_moving_update" (all layers in one launch: the record carries the first layer's name). */
int ursn_bn_set_frozen(ursn_net* net, int32_t on);

/* ---- loss weights made on the device (make_weights.hip) -------------------------------------------------------------------
 * Appended functions and one struct only: URSN_ABI_VERSION stays 9.
 * The per-voxel loss weight as a function of the label alone (the reference reads it as a stored larcv product,
 * config/input_train3d.cfg: Tensor3DProducer "weight"): per-event class balance plus a category of its own for the voxels where
 * two foreground classes meet.  For voxel v of event e:
 *   c(v) = (int)label[v] (truncation, like the dense head) if -1 < label[v] < ncls, else none (NaN included);
 *   v is a BOUNDARY voxel iff radius >= 1, c(v) >= 1 and some u != v inside the event's volume has max_i |u_i - v_i| <= radius in
 *     spatial coordinates, c(u) >= 1 and c(u) != c(v) (positions outside the volume, background and none voxels are never such a
 *     u; flat-index neighbours that are not spatial neighbours do not count; in 2-D the neighbourhood is a square);
 *   k(v) = ncls if v is boundary, else c(v); none voxels have no category;
 *   counts[e][k], k in 0..ncls = voxels of event e in category k;
 *   mode 0: w(v) = scale[k(v)];  mode 1: w(v) = (float)((double)scale[k(v)] / (double)counts[e][k(v)]) (one fp64 division, rounded
 *     once); none voxels get 0.0f. */
#define URSN_WEIGHTS_CLASS 0
#define URSN_WEIGHTS_INVFREQ 1
typedef struct ursn_make_weights_desc {
  int32_t ndim, spatial[3];   /* ndim 2 | 3 (spatial[2] unused in 2-D); prod(spatial) == voxels */
  int32_t n;                  /* events, 1..65535 */
  int64_t voxels;             /* per event, < 2^31 */
  int32_t ncls;               /* 1..8 */
  int32_t radius;             /* 0..3 (Chebyshev) */
  int32_t mode;               /* URSN_WEIGHTS_CLASS | URSN_WEIGHTS_INVFREQ */
  float scale[9];             /* [ncls + 1] read, finite: classes 0..ncls-1, then the boundary category */
} ursn_make_weights_desc;

/* label, weight_out [n, voxels] fp32 (device, 4-byte aligned, not overlapping); counts_out [n, ncls + 1] int64 (device) or NULL.
 * Three launches on `stream`: categorise box tiles (the tile and a radius-wide halo as one byte per voxel in LDS) into a byte map
 * and per-workgroup histograms in the scratch; reduce each event's histograms to counts and the ncls + 1 weight table; write the
 * weights from the map.  No atomics, no allocation, the scratch needs no initialisation, integer counts: the same arguments give
 * the same bits.  Enqueues only, never synchronises.  scratch: 8-byte aligned, >= ursn_make_weights_scratch_bytes(...), which is 0
 * for arguments out of domain.  Anything out of domain is refused with a message before any launch. */
int ursn_make_weights(const ursn_make_weights_desc* d, const float* label, float* weight_out, int64_t* counts_out, void* scratch,
                      size_t scratch_bytes, void* stream);
size_t ursn_make_weights_scratch_bytes(int32_t ndim, const int32_t* spatial, int32_t n, int32_t ncls, int32_t radius);

/* ---- guarded optimiser step (opt_guard.hip) ----------------------------------------------------------------------------------
 * Appended functions and three structs only: URSN_ABI_VERSION stays 9.
 * A deterministic segmented reduction over a flat fp32 gradient buffer, one segment per trainable tensor, and an Adam launch that
 * takes its decision (clip coefficient, skip) from the result on the device: no host round trip.  No atomics, no workgroup waits on
 * another, nothing is read that the same call or ursn_opt_state_init did not write, so the same arguments give the same bits.
 *
 * The STATE is caller-owned device memory (16-byte aligned, >= ursn_opt_state_size bytes; ursn_opt_state_layout gives the byte
 * offsets): a 64-byte header, the status record (ursn_opt_status), per-tensor results (ursn_opt_tensor[n_seg]), per-chunk fp64
 * partials (32 bytes per chunk), the segment table and the chunk table.  Segments are cut into chunks of URSN_OPT_CHUNK elements, a
 * segment's last chunk is ragged and a chunk never crosses a segment.
 *
 * Definitions (x finite: neither NaN nor +-Inf; a non-finite element contributes 0 to the sums and the maximum and is only
 * counted, so the sums stay comparable):
 *   per tensor   g_sumsq = sum (double)g * (double)g (each square exact), p_sumsq likewise over the parameters (0 without them),
 *                g_maxabs = max |g|, nonfinite = number of non-finite g;
 *   summation    inside a chunk a thread owns fixed elements, then lanes by shuffles, then waves in wave order; a tensor's chunks
 *                are added in chunk order, the tensors in index order;
 *   status       sumsq = sum over tensors of g_sumsq, norm = sqrt(sumsq) in fp64, nonfinite = total count;
 *   decision     coef = clip_norm > 0 && norm > clip_norm ? (float)((double)clip_norm / norm) : 1.0f  (fp64 division, rounded once),
 *                skip = skip_nonfinite && nonfinite > 0;
 *   update       on skip nothing is written to p, m or v.  Otherwise per element g' = g * coef (one fp32 multiply), then for tensors
 *                whose decay flag is set p' = p * decay (one fp32 multiply, rounded on its own) with
 *                decay = (float)(1.0 - (double)lr * (double)weight_decay) formed on the host (decoupled AdamW), then the Adam element
 *                update of ursn_adam with lr_t formed on the host from t exactly as ursn_adam forms it.  With coef == 1, no decay
 *                flag used (weight_decay == 0) and no skip the result equals ursn_adam's bit for bit.
 * The step counter: the host cannot know a skip without a synchronisation, so t advances on EVERY guarded call, skipped or not (a
 * skipped step costs one step of bias correction); skipped_total in the status record counts the skips.  A device-side pow would
 * keep t exact and lose the bit-equality with the unguarded path. */
#define URSN_OPT_CHUNK 4096
typedef struct ursn_opt_desc {
  float lr;               /* > 0 */
  float clip_norm;        /* <= 0: no clipping */
  float weight_decay;     /* 0: none; lr * weight_decay must lie in [0, 1] */
  int32_t skip_nonfinite; /* != 0: a step with any non-finite gradient element writes nothing */
} ursn_opt_desc;
typedef struct ursn_opt_status {
  double sumsq, norm;
  int64_t nonfinite;
  float coef;             /* 1.0f after a stats call, the clip coefficient after a decision */
  int32_t skip;           /* 0 after a stats call */
  int64_t calls;          /* decisions taken since ursn_opt_state_init */
  int64_t skipped_total;  /* of those, skips */
} ursn_opt_status;
typedef struct ursn_opt_tensor {
  double g_sumsq, p_sumsq;
  float g_maxabs;
  int32_t reserved_;      /* written 0 */
  int64_t nonfinite;
} ursn_opt_tensor;

/* Bytes of the state for n_seg tensors of nelem_host[i] elements; 0 for arguments out of domain (n_seg outside [1, 65536], an
 * element count < 1, 2^31 or more chunks).  No device access. */
size_t ursn_opt_state_size(const int64_t* nelem_host, int32_t n_seg);
/* out6 = {bytes, byte offset of the status record, of the per-tensor results, of the chunk partials, number of chunks,
 * URSN_OPT_CHUNK}.  No device access. */
int ursn_opt_state_layout(const int64_t* nelem_host, int32_t n_seg, int64_t* out6);
/* Builds the tables on the host, uploads them and zeroes the status record (cumulative counters included).  offsets_host /
 * nelem_host in floats from the start of the flat buffers, decay_host the per-tensor decay flags; segments must not overlap.
 * Synchronises (blocking copies), like ursn_create.  Too small or misaligned state and anything out of domain are refused. */
int ursn_opt_state_init(void* state, size_t bytes, const int64_t* offsets_host, const int64_t* nelem_host,
                        const int32_t* decay_host, int32_t n_seg);
/* Two launches on `stream`: one workgroup per chunk writes the chunk's partials, then ONE workgroup writes the per-tensor results
 * and the status record (coef 1.0f, skip 0; calls and skipped_total are kept).  g (and p when given) must cover every segment of
 * the table and be 4-byte aligned; 16-byte loads are used where a chunk's ADDRESS allows them.  Enqueues only. */
int ursn_opt_stats(void* state, const float* g, const float* p_or_null, void* stream);
/* One single-thread launch: sets coef and skip in the status record from what the preceding ursn_opt_stats left there, adds 1 to
 * calls and skip to skipped_total.  Enqueues only. */
int ursn_opt_decide(void* state, const ursn_opt_desc* desc, void* stream);
/* One launch over the chunk table: loads coef and skip from the status record and applies the update defined above for step t >= 1
 * (the caller's counter).  Chunks that do not lie inside [0, n) are not touched.  Enqueues only. */
int ursn_opt_adam(void* state, float* p, const float* g, float* m, float* v, int64_t n, const ursn_opt_desc* desc, int64_t t,
                  void* stream);
/* Copies the status record and (tensors_out != NULL) the n_seg per-tensor results to the host after everything enqueued on
 * `stream`: the ONLY synchronising call of this group besides the init. */
int ursn_opt_state_read(const void* state, int32_t n_seg, ursn_opt_status* status_out, ursn_opt_tensor* tensors_out, void* stream);

/* Net level, both plans alike (parameters, gradients and Adam slots are fp32 in both). */
/* Bytes of the state of a configuration's parameter list; no device access. */
int ursn_opt_state_bytes(const ursn_config* cfg, int64_t* out);
/* Builds the table from the handle's own parameter list (ursn_param order; decay flag = rank > 1, so BatchNorm beta is never
 * decayed) in the caller's buffer and attaches it; NULL detaches.  Synchronises like ursn_opt_state_init. */
int ursn_opt_attach(ursn_net* net, void* state, size_t bytes);
/* ursn_opt_stats over the handle's gradient buffer (and parameters when with_param_norms != 0).  Needs an attached state. */
int ursn_grad_stats(ursn_net* net, int32_t with_param_norms, void* stream);
/* Statistics, decision, Adam on `stream` (four launches), in place of ursn_apply_adam: advances the step counter by one on every
 * call, skipped or not (see above), and marks a pending ursn_forward_logits as ursn_apply_adam does.  desc->lr <= 0 means 1e-3 like
 * ursn_apply_adam, and lr_t is formed exactly as ursn_apply_adam forms it, so a neutral guarded step equals that call bit for bit.  Refused with a message when no state is attached. */
int ursn_apply_adam_guarded(ursn_net* net, const ursn_opt_desc* desc, void* stream);
/* ursn_opt_state_read on the attached state; tensors_out (or NULL) holds n_tensors records in ursn_param order. */
int ursn_opt_read(ursn_net* net, ursn_opt_status* status_out, ursn_opt_tensor* tensors_out, void* stream);

/* ---- tiling: crops of large voxel-list events and the way back (tiling.hip) --------------------------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * The network is built for one spatial size; real volumes are several times larger per axis.  The usual practice -- train on
 * crops, analyse a large event tile by tile and stitch -- done at the voxel-list boundary on the device: a LARGE batch (lists as in
 * ursn_voxel_batch, indices row-major in the shape `big`) goes up once, boxes of one size `tile` are cut out of it as a complete
 * ursn_voxel_batch at prod(tile) voxels per event, and the gather head's rows come back to the large event's own list order.
 *
 * Box b covers the voxels x of event box_event[b] with 0 <= x[a] - box_origin[b][a] < tile[a] on every axis a.  An origin may be
 * negative and a box may overhang the volume: what lies outside is background and contributes no entry.  Boxes may overlap, repeat
 * and be empty; a box whose event lies outside [0, n) is empty.  The CORE of a box, core_lo[b][a] <= x[a] - box_origin[b][a] <
 * core_hi[b][a] in box-local coordinates (NULL, NULL: the whole box), is the part whose voxels the box OWNS: with cores that
 * partition the volume every list entry is owned by exactly one box.
 *
 * All calls below enqueue only and never synchronise; no global atomics, the scratch needs no initialisation, the same arguments
 * give the same bits.  Null, misaligned, out-of-domain and too-small arguments are refused with a message before any launch. */
typedef struct ursn_crop_desc {   /* every pointer is a DEVICE pointer */
  int32_t ndim;                   /* 2 | 3 */
  int32_t big[3];                 /* shape of the large events, prod < 2^31 (big[2] unused in 2-D) */
  int32_t tile[3];                /* shape of every box, prod < 2^31 */
  int32_t n;                      /* large events, 1..65535 */
  int32_t boxes;                  /* B, 1..2^20 */
  int64_t m_total;                /* list entries the arrays below hold, < 2^31: positions at or beyond it are never read */
  const int64_t* offsets;         /* [n+1] as in ursn_voxel_batch */
  const int32_t* index;           /* [m_total] row-major in `big`, strictly increasing per event */
  const float* value;             /* [m_total]; value / label / weight / bg_weight may be NULL when no output asks for them */
  const float* label;
  const float* weight;
  const float* bg_weight;         /* [n] */
  const int32_t* box_event;       /* [B] */
  const int32_t* box_origin;      /* [B, ndim] */
  const int32_t* core_lo;         /* [B, ndim] box-local, or NULL together with core_hi */
  const int32_t* core_hi;
} ursn_crop_desc;

/* count_out[b] = list entries inside box b, owned_out[b] = of those, entries inside its core: int64 [B] each (device).  Three
 * launches: per box the contiguous range of the event's list that its slowest-axis slab covers (two binary searches), per part of
 * that range the counts (wave64 ballot / popcount), per box their sum in part order.
 * scratch: 8-byte aligned, >= ursn_crop_scratch_bytes(ndim, big, tile, boxes), which is 0 for arguments out of domain. */
int ursn_crop_count(const ursn_crop_desc* d, int64_t* count_out, int64_t* owned_out, void* scratch, size_t scratch_bytes,
                    void* stream);
size_t ursn_crop_scratch_bytes(int32_t ndim, const int32_t* big, const int32_t* tile, int32_t boxes);

typedef struct ursn_crop_out {    /* DEVICE pointers; a complete ursn_voxel_batch of B events at prod(tile) voxels, plus src / owned */
  int64_t* offsets;               /* [B+1], offsets[0] = 0: the TRUE counts, whatever cap is */
  int32_t* index;                 /* [cap] box-local row-major index, strictly increasing per box */
  float* value;                   /* [cap] gathered from the large list; value / label / weight each optional (NULL) */
  float* label;
  float* weight;                  /* together with bg_weight */
  float* bg_weight;               /* [B] bg_weight[b] = d->bg_weight[box_event[b]] (0 for a box of an event outside [0, n)) */
  int32_t* src;                   /* [cap] position of the entry in the large list (optional) */
  uint8_t* owned;                 /* [cap] 1: the entry lies inside the box's core, else 0 (optional) */
  int64_t cap;                    /* entries whose position is >= cap are never written (ursn_labels_to_voxels' convention) */
} ursn_crop_out;

/* The boxes of d as one voxel batch: the range and count launches of ursn_crop_count, a one-workgroup scan in box order, and the
 * write pass -- a stable compaction of each box's range, so every box's list is sorted without a sort.  A run of a longer box list
 * is that list's arrays at an offset.  The result is what ursn_voxels_to_dense, ursn_voxels_to_dense_sym and ursn_infer_voxels take
 * as it is.  Scratch as for ursn_crop_count. */
int ursn_crop_write(const ursn_crop_desc* d, const ursn_crop_out* out, void* scratch, size_t scratch_bytes, void* stream);

/* After ursn_infer_voxels on a crop batch: rows j < m with owned[j] == 1 are copied to row src[j] of the outputs, which are laid
 * out in the large batch's list order (scores_out [rows_out, ncls] fp32, pred_out / ana_out [rows_out] uint8).  Rows that are not
 * owned, or whose src lies outside [0, rows_out), write nothing.  Each (input, output) pair is optional and comes together, not all
 * three absent.  With cores that partition the volume every output row is written exactly once over all crop batches: no atomics,
 * and the order of the batches does not matter.  One launch; m = 0 launches nothing. */
int ursn_scores_scatter(const int32_t* src, const uint8_t* owned, int64_t m, int32_t ncls, const float* scores,
                        const uint8_t* pred, const uint8_t* ana, float* scores_out, uint8_t* pred_out, uint8_t* ana_out,
                        int64_t rows_out, void* stream);

/* ---- frozen-BatchNorm training (elementwise.hip, bf16_elementwise.hip) ----------------------------------------------------------
 * Appended functions only: URSN_ABI_VERSION stays 9.
 * Fine-tuning on FIXED statistics: the forward is the frozen one of ursn_bn_set_frozen, and the backward differentiates through
 * constants mean / rstd instead of through a batch's moments.  With g = dy * relu-mask
 *     dz = rstd * g        d(beta) += sum g        (join: dz2 = rstd2 * g, d(beta2) += sum g;  dres (=|+=) g)
 * -- both projection terms of the batch form, mean(g) and xhat * mean(g * xhat), are gone (beta stays trainable).  Where a layer's
 * BatchNorm backward ran as a reduce pass and an apply pass it is ONE pass that reads g and what the mask needs (y, or z for
 * bn(z) > 0 with the forward's own fmaf, or the mask bits / bytes), writes dz and sums g per channel on the way; the sum goes through
 * the batch form's partials and finalise, in its order, so d(beta) has the same bits on either route.  Where the sums come out of
 * the epilogue of the kernel that produced dy, or dz is formed on load by the layer's data-gradient kernel, those kernels run
 * unchanged and the finalise hands them zero means.  URSN_BN_FROZEN_FUSED=0 (A/B) takes that second route everywhere.
 * When profiling, the single pass is recorded under pass id 5 as "bn_bwd_frozen" / "bbn_bwd_frozen" with the bytes it moves.
 *
 * ursn_bn_frozen_train: on != 0 lets the training entries run while the handle is frozen -- ursn_accum_step, ursn_forward_logits and
 * ursn_backward_logits, on both plans -- with the frozen forward and the derivative above.  Refused with a message unless the handle
 * is frozen (ursn_bn_set_frozen); ursn_bn_set_frozen(net, 0) clears it.  ursn_bn_update stays refused after such a forward (its mean
 * / rstd are the moving statistics), a step in this mode never enters or replays a URSN_GRAPH graph, and a pending
 * ursn_forward_logits does not survive a change of this setting.  Host state only: no launch, no synchronisation. */
int ursn_bn_frozen_train(ursn_net* net, int32_t on);
/* Op level, fp32: g = dy * (relu ? mask : 1) with mask = y > 0 (y given) or bn(z) > 0 (y NULL: z, mean, rstd, beta given);
 * dz = rstd * g, dbeta += sum g.  Compact [voxels, channels] tensors; z, mean and beta may be NULL where the mask does not need
 * them.  scratch >= ursn_bn_scratch_bytes(voxels, channels).  Two launches, enqueues only. */
int ursn_bn_backward_frozen(const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                            const float* beta, float* dz, float* dbeta, int64_t voxels, int32_t channels, int32_t relu,
                            void* scratch, size_t scratch_bytes, void* stream);
/* Op level, bf16: ursn_bn_bf16_backward's descriptor, unchanged, with its mean / rstd (mean2 / rstd2) used as given; the single pass
 * reads z only for the bn(z) > 0 mask and z2 never.  scratch >= ursn_bn_bf16_scratch_bytes(voxels, channels). */
int ursn_bn_bf16_backward_frozen(const ursn_bn_bf16_desc* d, void* scratch, size_t scratch_bytes, void* stream);

/* MFMA lane-layout probe used by tests (writes 64*16 floats). */
int ursn_mfma_probe(int32_t which, float* out, void* stream);

/* ---- statistics scratch of ursn_conv_forward_stats (conv_api.hip) --------------------------------------------------------------
 * Appended function only: URSN_ABI_VERSION stays 9.
 * Exactly the number ursn_conv_forward_stats compares its scratch_bytes against for this descriptor: the partial-sum rows of the
 * kernel family the descriptor dispatches to (same predicate chain as the call, dtype 1 included), or the separate reduction's
 * buffer for the shapes no fused-statistics kernel takes.  A multiple of 8; 0 where the call refuses the descriptor for another
 * reason (bf16 transposed convs, a fused form the shape has no kernel for, a forced algo that does not take the shape).  Host logic
 * only: no device access. */
size_t ursn_conv_stats_scratch_bytes(const ursn_conv_desc* d);

/* ---- device loss head (loss_head.hip) ---------------------------------------------------------------------------------------
 * Appended functions and one struct only: URSN_ABI_VERSION stays 9.
 * A second head beside the reference's weighted softmax cross-entropy: focal exponent, label smoothing and a batch soft-Dice term,
 * computed from conv2's stored operands straight into the plan's d(logits) tensor; no dense logits tensor exists.  Per voxel p with
 * logits z, q = softmax(z), C = ncls, l = (int)label[p] (truncated toward zero), w = weight[p] (1 without a weight), P = n * voxels:
 *     t_k   = (1 - smoothing) [k == l] + smoothing / C            ce_p = -sum_k t_k log q_k          f_p = (1 - q_l)^gamma
 *     L_ce  = (1/n) sum_p w_p f_p ce_p                            (sum over voxels, mean over events: the reference's reduction)
 *     I_c = sum_p q_pc [l_p == c], S_c = sum_p q_pc, Y_c = sum_p [l_p == c]      (all P voxels of the batch, unweighted)
 *     L_dice = 1 - (1/C) sum_c (2 I_c + dice_eps) / (S_c + Y_c + dice_eps)       L = L_ce + dice_weight * L_dice
 * A voxel with l == ignore_label adds nothing to L_ce, the Dice sums or d L / d z (its stored gradient is zero) but still counts in
 * the accuracies; any other label outside [0, C) makes the loss NaN, as in the head.
 * Domain: gamma == 0 or gamma >= 1 (finite), 0 <= smoothing < 1, dice_weight >= 0 (finite), dice_eps > 0 (finite); ignore_label -1:
 * none.  With gamma == 0, smoothing == 0, dice_weight == 0 and ignore_label == -1 the kernel takes the heads' own statements and its
 * stored dlogits, metrics and BatchNorm-backward partials carry the bits of head_kernel (fp32 z: expf / logf) or bhead_kernel (bf16
 * z: the fast __expf / __logf; every other spec uses expf / logf on either dtype). */
typedef struct ursn_loss_desc {
  double gamma, smoothing, dice_weight, dice_eps;
  int32_t ignore_label;
} ursn_loss_desc;

/* d: n, voxels, ncls, z / z_cstride / dtype, mean / rstd / beta as in ursn_logits_dense, data [n, voxels] or NULL (acc_nonzero is
 * NaN without it); offsets / index unused.  label [n, voxels] fp32, weight nullable.
 * dlog_out (NULL: loss and metrics only), in the three layouts of ursn_dlogits_pack: out_dtype 0 with out_cstride 4, <= 4 classes and
 * 16-byte alignment: one 16-byte store, pad lanes zero; any other fp32 stride >= ncls: the ncls values only; out_dtype 1: stride 8,
 * 16-byte aligned, bf16 round-to-nearest-even, pad lanes zero.
 * bs_partial_or_null: the logits layer's BatchNorm-backward partials from the STORED dlogits, [bs_blocks][3][C] doubles, third row
 * zero, C = 4 (fp32: z and dlog_out both at stride 4, <= 4 classes, 16-byte aligned) or 8 (bf16 z and bf16 dlog_out); needs mean /
 * rstd and bs_blocks == the head's block count for (n, voxels).
 * out8 (device, 4-byte aligned) = {loss, acc_all, acc_nonzero, n_nonzero, ce_term, dice_term, 0, 0}.
 * One thread per voxel, grid-stride over the heads' workgroups of 256; fp64 partials per block, a one-workgroup finalise with a
 * fixed tree; no atomics; the scratch needs no initialisation; the same arguments give the same bits.  dice_weight == 0: two
 * launches (main, finalise); otherwise four at most (sums, finalise, gradient).  scratch: 8-byte aligned, >=
 * ursn_loss_head_scratch_bytes(n, voxels, ncls) (0 for n outside [1, 65535], voxels outside [1, 2^31) or ncls outside [1, 8]).
 * Null, misaligned, out-of-domain and too-small arguments are refused before any launch.  Enqueues only. */
size_t ursn_loss_head_scratch_bytes(int32_t n, int64_t voxels, int32_t ncls);
int ursn_loss_head(const ursn_vscores_desc* d, const float* label, const float* weight, const ursn_loss_desc* spec, void* dlog_out,
                   int32_t out_cstride, int32_t out_dtype, double* bs_partial_or_null, int32_t bs_blocks, float* out8, void* scratch,
                   size_t scratch_bytes, void* stream);

/* ursn_accum_step with the loss head in place of the plan's head: forward() exactly as a step calls it, ursn_loss_head on conv2's
 * operands into the handle's d(logits) tensor (with the BatchNorm-backward partials under the conditions the plan's head carries
 * them), the unchanged backward; gradients are ADDED to the flat buffer and the metrics land where ursn_read_metrics reads them.
 * Both plans; a training entry (refused while frozen unless ursn_bn_frozen_train is on); ends a pending ursn_forward_logits like
 * every run call; never enters or replays a URSN_GRAPH graph.  Recorded as pass 6 "losshead" / "losssums" / "lossfinal" when
 * profiling.  Enqueues only.  ursn_eval_loss: the same without dlogits and backward (forward-only: legal while frozen). */
int ursn_accum_step_loss(ursn_net* net, const float* data, const float* label, const float* weight, int32_t n,
                         const ursn_loss_desc* spec, void* stream);
int ursn_eval_loss(ursn_net* net, const float* data, const float* label, const float* weight, int32_t n, const ursn_loss_desc* spec,
                   void* stream);
/* out2 = {ce_term, dice_term} of the last ursn_accum_step_loss / ursn_eval_loss on this handle.  Synchronises the stream. */
int ursn_read_loss_terms(ursn_net* net, float* out2, void* stream);

/* ---- work partition of an op-level conv call (conv_api.hip) ----------------------------------------------------------------------
 * Appended function only: URSN_ABI_VERSION stays 9.
 * The work split the family ursn_conv_plan names would take for this descriptor / pass (0 forward, 1 data gradient, 2 weight
 * gradient), read from the plan function the family's launcher itself calls, under the environment switches of this process.
 * Host logic only: no device access.  out = {workgroups of the main launch, sequential steps per workgroup along the marched or
 * looped axis, partial results reduced afterwards (0: none), a family-specific word}:
 *   dconv    {boxes * tiles * gsplit * cout blocks, chunk rounds per workgroup, split-K slabs (0: gsplit 1), SLAB flag}; SLAB 0: the
 *            forward's statistics partials are workgroups * 128 doubles, written by the conv kernel itself
 *   pconv    {workgroups (capped), 256-voxel steps of the first workgroup, rows of statistics partials (forward), voxels of the last step}
 *   b3conv   {workgroups, planes per z segment, rows of statistics partials, z segments}
 *   bcbconv  {workgroups, planes per z segment, rows of statistics partials per cout block, z segments}
 *   bdconv   {workgroups, chunk rounds per workgroup, split-K slabs (0: gsplit 1), box voxels}
 *   bconv    {workgroups, boxes a workgroup walks, rows of statistics partials per cout block, box voxels * 10 + stage buffers (1 or
 *            2)} -- of the first non-empty parity class where a stride-2 pass runs one launch per class
 *   bsconv   {workgroups, 32-channel chunks a workgroup contracts, rows of statistics partials per cout block, coarse box voxels}
 *   b3wgrad  {workgroups = slabs written, planes per column, slabs the reduce kernel walks (after the fold), fold group (0: no fold)}
 *   bdwgrad  {workgroups, boxes a workgroup walks, slabs per channel block, boxes}: the last slice is short when boxes % steps != 0
 *   bwgrad   {workgroups, boxes a workgroup walks, slabs per channel block, box voxels}
 *   tconv    {workgroups of one launch (a channel-blocked layer runs several such launches), planes per z segment, rows of
 *            statistics partials (forward: one per workgroup), z segments}
 *   twgrad   {workgroups of one launch, planes per z segment AFTER the plane-pair round-up of the Cout = 8 form, slabs reduced
 *            afterwards (two per workgroup in the plane-pair form, else one), z segments + 2^32 when the round-up changed the
 *            segment ursn_pick_zseg had picked (bit 32: the picked segment was odd and there is more than one)}
 *   tdeconv  (also "tdeconv+pw") {workgroups of one launch, LOW-resolution planes per z segment, rows of statistics partials
 *            (forward), z segments}
 *   vwgrad   {workgroups, planes per z segment, slabs reduced afterwards, z segments}
 *   b0conv   {workgroups, planes per z segment, rows of statistics partials (one per workgroup), z segments}
 *   b0wgrad  {workgroups, planes per z segment, slabs reduced afterwards, z segments}
 * In every z-marching family the last segment of a column is short when Z % planes != 0.  The resident-slot count the tiled families
 * and the persistent box walks divide by is occupancy * CUs of the device; URSN_CU_COUNT=n (1..1024, tests) replaces the device's count.
 * Every other family (their splits have no plan struct, or no switch moves them): returns non-zero, "not reported". */
int ursn_conv_partition(const ursn_conv_desc* d, int32_t pass, int64_t out[4]);

/* ---- voxel clusters: connected components of a voxel list (cluster.hip) -----------------------------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * The step every consumer takes after the per-voxel class: touching voxels become track and shower clusters, small fragments are
 * dropped.  Done on the sorted per-event lists themselves (ursn_voxel_batch's offsets / index, row-major in `spatial`: the network's
 * shape, or `big` of a tiled event), so time and scratch scale with the list and never with the volume.
 *
 * An entry PARTICIPATES when its index lies in [0, prod(spatial)) and bit cls[j] of class_mask is set (a class >= 32 never does).
 * Two participating entries of ONE event are joined when their coordinates differ by at most 1 on every axis and in at most A axes:
 * 3-D connectivity 6 | 18 | 26 is A = 1 | 2 | 3, 2-D connectivity 4 | 8 is A = 1 | 2; with same_class they must also have equal
 * class.  Adjacency is decided on coordinates: linear indices that differ by 1 across a row end, or by one row across a plane end,
 * are not neighbours.  Clusters are the connected components of that relation with at least min_size entries, numbered per event
 * from 0 in the order of their lowest list position (scipy.ndimage.label's numbering for a raster-ordered list).  Every other entry
 * gets cluster -1.  Events without entries are legal; entries of different events never join.
 * Per-cluster table (optional): first = the cluster's lowest list position counted from its event's first entry (a list position,
 * not a voxel index), size = its entry count, cls = the class of `first`.
 *
 * Method: union-find over list positions.  Neighbours are found by binary searches confined to the event's range of the list and
 * the consecutive entries of the neighbouring row; links are made with 32-bit integer atomicMin and sizes summed with 32-bit integer
 * atomicAdd in global memory.  The outputs do not depend on arrival order: every link points from a higher position to a lower one,
 * so a component's representative is its lowest list position whatever order the merges land in, and sizes are integer sums.  No
 * float atomics.  Every device loop is bounded (parent pointers only decrease, each loop carries a trip cap taken from the list
 * length); a thread that exceeds one sets *status non-zero and leaves -- the outputs are then not valid.  The ids are formed in a
 * later launch than the merges.  Seven launches; enqueues only, never synchronises; the scratch needs no initialisation; the same
 * arguments give the same bits.  Null, misaligned, out-of-domain and too-small arguments are refused with a message before any
 * launch; m_total = 0 launches one kernel that writes count, table_offsets and status and reads no list. */
typedef struct ursn_cluster_desc {      /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* shape the indices are row-major in, prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int64_t m_total;                      /* list entries, < 2^31; positions at or beyond it are never read or written */
  const int64_t* offsets;               /* [n+1] as in ursn_voxel_batch */
  const int32_t* index;                 /* [m_total] strictly increasing per event */
  const uint8_t* cls;                   /* [m_total] class of each entry (pred, ana, or a true label) */
  int32_t connectivity;                 /* 3-D: 6 | 18 | 26;  2-D: 4 | 8 */
  uint32_t class_mask;                  /* bit k: entries of class k take part; all others get cluster -1 */
  int32_t same_class;                   /* 1: only entries of equal class join;  0: any two participating entries */
  int32_t min_size;                     /* >= 1: components with fewer entries are dropped (cluster -1) and not numbered */
} ursn_cluster_desc;

typedef struct ursn_cluster_out {       /* DEVICE pointers */
  int32_t* cluster;                     /* [m_total] event-local id 0..K_e-1, or -1 */
  int32_t* count;                       /* [n] K_e */
  int32_t* first; int32_t* size; uint8_t* cls;   /* optional per-cluster table, [cap] each, events back to back in id order */
  int64_t* table_offsets;               /* [n+1], needed iff a table array is given; true counts whatever cap is */
  int64_t cap;                          /* table rows at or beyond cap are never written */
  int32_t* status;                      /* [1] 0, or non-zero if a bounded device loop ran out */
} ursn_cluster_out;

/* Bytes of scratch for a list of m_total entries: 8-byte aligned, at least 8; 0 for n outside [1, 65535] or m_total outside
 * [0, 2^31).  Host logic only. */
size_t ursn_cluster_scratch_bytes(int32_t n, int64_t m_total);
int ursn_cluster_voxels(const ursn_cluster_desc* d, const ursn_cluster_out* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- per-cluster object records: moments, principal axis, end points (cluster_features.hip) -------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * What a consumer takes from a cluster: its charge, position, direction, extent and its two ends, each a reduction over the
 * cluster's members.  Input: the lists ursn_cluster_voxels read, the ids and table_offsets it wrote, and optionally the value list.
 * The members of table row r = table_offsets[e] + id are the entries j of event e with cluster[j] == id; coordinates x[0..2] are the
 * row-major coordinates of index[j] in `spatial` (2-D: x[2] = 0).  uresnet_amd/clusters.py (cluster_features_numpy) states every
 * field operation by operation; the device gives the same bits.
 *
 * int64 table, URSN_CLFEAT_I columns per row:
 *   [0] n            members
 *   [1] charge       sum of rint((double)value * 2^16); a member with |value| >= 2^15 or a non-finite value adds nothing and sets
 *                    bit 0 of flags; no value list: 0
 *   [2..4] s         coordinate sums            [5..7] lo, [8..10] hi   bounding box
 *   [11..13] m       anchor floor((2 s + n) / (2 n)): the centroid rounded to a voxel
 *   [14..16] d       sum (x - m)                [17..22] dd   sum (x_a - m_a)(x_b - m_b) for ab = 00, 11, 22, 01, 02, 12
 *   [23] flags       [24] end_lo, [25] end_hi   list positions (global across the batch) of the members with the smallest / largest
 *                    projection on the axis, the lower position among equals in both
 * With every extent <= 32768 and m_total < 2^31: |s|, |d| < 2^46, |dd| < 2^61, |charge| <= 2^62.
 * fp64 table, URSN_CLFEAT_R columns per row (every value one correctly rounded operation after another, never contracted):
 *   [0..2] centroid  s / n
 *   [3..8] cov       dd[ab] / n - (d[a] / n) * (d[b] / n), same order as dd; |d / n| <= 0.5 by the anchor, so nothing cancels
 *   [9..11] eval     eigenvalues of cov, descending: cyclic Jacobi, a fixed 8 sweeps over (0,1), (0,2), (1,2), Rutishauser's rotation
 *   [12..14] axis    unit eigenvector of eval[0], its component of largest magnitude positive
 *   [15] length      t_hi - t_lo      [16] t_lo, [17] t_hi   the extreme projections: fp32 values, stored widened
 * where a member's projection is t = (axis[0] (x0 - m0) + axis[1] (x1 - m1)) + axis[2] (x2 - m2) in fp64, rounded once to fp32.
 *
 * Method: per-entry passes accumulate with 64-bit INTEGER atomics (add / min / max, agent scope) and nothing else, so no result
 * depends on arrival order; the end-point search packs (order-preserving code of the fp32 projection) << 32 | position into one
 * 64-bit atomic min, and the same code with the complemented position into one atomic max.  Equal-id lanes next to each other in a
 * wave are combined first, then the runs of a workgroup in an LDS table: one global atomic per field and distinct row of a workgroup
 * (URSN_CLFEAT_WAVE=0: one per field and entry; same bits).  Per-cluster passes stride up to the count they read from
 * table_offsets[n].  Seven launches; enqueues only, never synchronises; the scratch needs no
 * initialisation; every device loop is bounded.  Skipped: entries with cluster == -1 and entries whose row is >= cap.  An entry
 * with an id whose index lies outside [0, prod(spatial)), whose id lies outside its event's rows, or a row without members sets
 * *status non-zero (none can come from ursn_cluster_voxels) and is skipped.  Rows at or beyond cap are never written.  Null,
 * misaligned, out-of-domain and too-small arguments are refused with a message before any launch; m_total = 0 or no clusters
 * still writes *status. */
#define URSN_CLFEAT_I 26   /* int64 columns:  208 bytes per row */
#define URSN_CLFEAT_R 18   /* fp64 columns:   144 bytes per row */

typedef struct ursn_cluster_feat_desc { /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t reserved;                     /* 0 */
  int64_t m_total;                      /* list entries, < 2^31 */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] */
  const float* value;                   /* [m_total], or null: charge = 0 */
  const int32_t* cluster;               /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets;         /* [n+1] as ursn_cluster_voxels wrote it */
} ursn_cluster_feat_desc;

typedef struct ursn_cluster_feat_out {  /* DEVICE pointers */
  int64_t* itab;                        /* [cap][URSN_CLFEAT_I] */
  double* rtab;                         /* [cap][URSN_CLFEAT_R] */
  int64_t cap;                          /* rows at or beyond cap are never written */
  int32_t* status;                      /* [1] 0, or non-zero: an entry or a row was inconsistent */
} ursn_cluster_feat_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535], m_total outside [0, 2^31) or cap < 0.  Host logic only. */
size_t ursn_cluster_features_scratch_bytes(int32_t n, int64_t m_total, int64_t cap);
int ursn_cluster_features(const ursn_cluster_feat_desc* d, const ursn_cluster_feat_out* out, void* scratch, size_t scratch_bytes,
                          void* stream);

/* ---- cluster matching: the contingency table of two clusterings of the same lists (cluster_match.hip) ---------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * The step between "objects" and "evaluation": are the predicted clusters the true ones?  Input: two id arrays over the same
 * concatenated per-event lists, each as ursn_cluster_voxels writes them (event-local id or -1) with its table_offsets, and
 * optionally the value list.  Side A is "predicted" and side B "true" by convention; the definition is symmetric.
 * uresnet_amd/clusters.py (cluster_match_numpy) states every field operation by operation; the device gives the same bits.
 *
 * A CELL is a pair (A row, B row) of one event with at least one common entry: c = the number of common entries, q = the sum of
 * rint((double)value * 2^16) over them (the charge rule of the object records: an entry with |value| >= 2^15 or a non-finite
 * value adds nothing and sets bit 0 of the flags of both its rows; no value list: 0).
 *
 * Row record, one per row of each side (X the row's side, Y the other).  int64, URSN_CLMATCH_I columns:
 *   [0] n         members of the row, whatever their Y id       [1] charge    fixed-point sum over the members
 *   [2] matched   members whose Y id is >= 0                     [3] partners  cells of the row
 *   [4] best      event-local Y id of the cell with the largest c, the lowest id among equals; -1 without a cell
 *   [5] overlap   that cell's c (0 without a cell)               [6] overlap_charge   that cell's q
 *   [7] flags     bit 0: a charge was dropped; bit 1: mutual (the best row's own best is this row)
 * fp64, URSN_CLMATCH_R columns, each ONE correctly rounded division of integers converted to fp64:
 *   [0] purity = overlap / n      [1] efficiency = overlap / n_Y(best)      [2] iou = overlap / (n + n_Y(best) - overlap)
 *   [3] matched / n               ([1] and [2] are 0.0 without a cell)
 * Event record, one per event.  int64, URSN_CLMATCH_EI columns:
 *   [0] N = entries with both ids >= 0      [1] S = sum over cells of c (c - 1) / 2
 *   [2] SA = sum over A rows of matched (matched - 1) / 2      [3] SB = the same over B rows
 *   [4] cells   [5] KA   [6] KB   [7] mutual pairs
 *   [8] sum over A rows of overlap   [9] sum over A rows of n   [10], [11] the same over B rows
 * (with m_total < 2^31 every one of them is below 2^62).  fp64, URSN_CLMATCH_ER columns:
 *   [0] adjusted Rand index: P = N (N - 1) / 2; 1.0 if P == 0; E = (f(SA) * f(SB)) / f(P); mean = (f(SA) + f(SB)) * 0.5;
 *       den = mean - E; 1.0 if den == 0; else (f(S) - E) / den   (f = int64 -> fp64; one rounded operation each, never contracted)
 *   [1] [8] / [9], 0.0 when [9] == 0      [2] [10] / [11], 0.0 when [11] == 0      [3] f(2 mutual) / f(KA + KB), 0.0 without rows
 * Cell list (optional), CSR by global A row: pair_offsets[r] .. pair_offsets[r + 1] are the cells of A row r in ascending B id;
 * pair_b = event-local B id, pair_n = c, pair_q = q.
 *
 * Method: every entry's (A row, B row) pair -- a missing side counts as a row of its own kind -- is counted in an open-addressing
 * table in the scratch (64-bit keys claimed by compare-and-swap, count and charge by 64-bit INTEGER atomic adds, agent scope); a pass
 * over the slots spreads each cell onto its two rows (integer adds, and ONE packed 64-bit atomic max per side for `best`:
 * c << 32 | 0xFFFFFFFF - other row, so equal counts fall to the lower id); one thread per row writes the records; the event sums
 * are integer adds; the cell list is an exclusive scan of `partners`, a drop into the row's segment at an atomic cursor and a rank
 * by B id inside the segment.  Which slot a cell lands in depends on arrival order; nothing that is output does.  No float atomics.
 * Equal-pair lanes next to each other in a wave are combined first, then the runs of a workgroup in an LDS table: one insertion per
 * distinct pair of a workgroup (URSN_CLMATCH_WAVE=0: one insertion per entry; same bits).  Every device loop is bounded (a probe
 * walk by the slot count, an event search by 17 halvings, a rank by `partners`).  Enqueues only, never synchronises; the scratch needs
 * no initialisation; the same arguments give the same bits.
 * *status is 0, or non-zero when an id lies outside [-1, K_e) of its event, a row has no member, the offsets are not those of the
 * lists, or a bounded loop ran out (none can come from ursn_cluster_voxels); such an entry or row is skipped.  Rows at or beyond
 * cap_a / cap_b and cells at or beyond pair_cap are never written; every row and cell below them is complete whatever the caps
 * are, and pair_offsets holds the true counts.  m_total = 0 or no rows still writes *status, the event records and pair_offsets[0].
 * Null, misaligned, out-of-domain and too-small arguments are refused with a message before any launch. */
#define URSN_CLMATCH_I 8    /* int64 columns of a row record */
#define URSN_CLMATCH_R 4    /* fp64 columns of a row record */
#define URSN_CLMATCH_EI 12  /* int64 columns of an event record */
#define URSN_CLMATCH_ER 4   /* fp64 columns of an event record */

typedef struct ursn_cluster_match_desc { /* every pointer is a DEVICE pointer */
  int32_t n;                            /* events, 1..65535 */
  int32_t reserved;                     /* 0 */
  int64_t m_total;                      /* list entries, < 2^31 */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* cluster_a;             /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets_a;       /* [n+1] */
  const int32_t* cluster_b;             /* [m_total] */
  const int64_t* table_offsets_b;       /* [n+1] */
  const float* value;                   /* [m_total], or null: every charge is 0 */
} ursn_cluster_match_desc;

typedef struct ursn_cluster_match_out { /* DEVICE pointers */
  int64_t* a_int;                       /* [cap_a][URSN_CLMATCH_I] */
  double* a_real;                       /* [cap_a][URSN_CLMATCH_R] */
  int64_t cap_a;                        /* A rows at or beyond it are never written */
  int64_t* b_int;                       /* [cap_b][URSN_CLMATCH_I] */
  double* b_real;                       /* [cap_b][URSN_CLMATCH_R] */
  int64_t cap_b;
  int64_t* event_int;                   /* [n][URSN_CLMATCH_EI] */
  double* event_real;                   /* [n][URSN_CLMATCH_ER] */
  int64_t* pair_offsets;                /* [cap_a + 1], or null: no cell list; entries 0 .. min(KA_total, cap_a) are written */
  int32_t* pair_b;                      /* [pair_cap] each, or all three null: the counts in pair_offsets only */
  int64_t* pair_n;
  int64_t* pair_q;
  int64_t pair_cap;                     /* cells at or beyond it are never written */
  int32_t* status;                      /* [1] */
} ursn_cluster_match_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535], m_total outside [0, 2^31) or a cap < 0.  Host logic only. */
size_t ursn_cluster_match_scratch_bytes(int32_t n, int64_t m_total, int64_t cap_a, int64_t cap_b, int64_t pair_cap);
int ursn_cluster_match(const ursn_cluster_match_desc* d, const ursn_cluster_match_out* out, void* scratch, size_t scratch_bytes,
                       void* stream);

/* ---- cluster contact graph: which clusters lie near each other, and the interaction groups they form (cluster_graph.hip) ---------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * The step from objects to relations to groups.  Input: the lists ursn_cluster_voxels read, the ids and table_offsets it wrote,
 * optionally the value list and the cluster table's cls.  uresnet_amd/clusters.py (cluster_graph_numpy) states every field; the
 * device gives the same bits.  Every quantity is an integer.
 *
 * Coordinates x[0..2] are the row-major coordinates of index[j] in `spatial` (2-D: x[2] = 0).  Two entries of one event are NEAR
 * when each has an id >= 0, the ids differ and the coordinates differ by at most `gap` on every axis (Chebyshev distance, decided on
 * coordinates: never across a row end, a plane end or an event boundary).  An EDGE is an unordered pair of rows a < b of one event
 * with at least one near pair of entries, one in a and one in b.
 *
 * Edge record, URSN_CLGRAPH_E int64, CSR by global row a (edge_offsets[r] .. edge_offsets[r + 1], ascending b):
 *   [0] b       event-local id of the higher row           [1] pairs   unordered near pairs of entries between the two rows
 *   [2] touch   those at Chebyshev distance 1              [3] dist2   the smallest squared Euclidean distance over the near pairs
 *   [4] pos_a   [5] pos_b   list positions (in the whole batch) of the near pair smallest in (dist2, position in a, position in b)
 * Row record, URSN_CLGRAPH_I int64:
 *   [0] degree  edges of the row, on either side           [1] group   event-local group id
 *   [2] nearest event-local id of the partner smallest in (dist2, id); -1 without an edge      [3] nearest_dist2 (0 without one)
 *   [4] pairs   summed over the row's edges                [5] touching   edges of the row with touch > 0
 * GROUPS are the connected components of an event's rows under its edges (a row without an edge is a group of its own), numbered
 * per event in the order of their lowest row id.  Group record, URSN_CLGRAPH_G int64, with group_offsets[n + 1]:
 *   [0] rows   [1] edges   [2] n = member entries   [3] charge = sum of rint((double)value * 2^16) (|value| >= 2^15 or a non-finite
 *   value adds nothing and sets bit 0 of the flags; no value list: 0)   [4..6] lo   [7..9] hi (the coordinate box, 0 for the missing
 *   2-D axis)   [10] first_row   [11] class_mask | flags << 32 (bit cls of every member row; cls must be < 32; no cls: 0)
 * Event record, URSN_CLGRAPH_EV int64: [0] groups   [1] edges   [2] isolated (rows of degree 0)   [3] the largest group's n.
 * Per entry: group int32 = the event-local group of the entry's row, -1 for id -1.
 *
 * Bounds: every entry has at most (2 gap + 1)^3 - 1 = 342 neighbours and each pair is counted once, so pairs < m_total * 171 < 2^39
 * in an edge, a row or summed over all; dist2 <= 3 * 3^2 = 27; box coordinates are below 2^15; |charge| <= 2^31 * 2^31 = 2^62.
 *
 * Method: one thread per entry visits the 5 / 13 / 25 rows of the volume before its own within +-gap and the left part of its own
 * row, one binary search (<= 32 halvings) and at most 2 gap + 1 consecutive entries each: every unordered pair once, from its higher
 * list position, no dense map.  Edges are counted in an open-addressing table in the scratch, a power of two >= 2 edge_cap + 2
 * slots, keyed (row a << 32) | row b: 64-bit compare-and-swap claims and 64-bit INTEGER atomic adds at agent scope; the closest pair
 * is ONE packed 64-bit atomic minimum (dist2 << 40 | pos_a << 9 | code of x_b - x_a, which orders pos_b), pos_b is found again by a
 * binary search.  Equal-edge lanes next to each other in a wave are combined first, then the edges of a workgroup in a 256-slot LDS
 * table that falls through to direct insertions when full (URSN_CLGRAPH_WAVE=0: one insertion per near pair; same bits).  Groups:
 * union-find over global rows with 32-bit atomicMin links to the lower root, flatten, count / one-workgroup scan / rank; group
 * records by 64-bit integer adds, minima, maxima and ors.  Edge list: scan, drop, rank by b.  No float atomics.  Enqueues only, never
 * synchronises; the scratch needs no initialisation; every device loop is bounded; the same arguments give the same bits.
 *
 * *status is 0, or: bit 0 an id outside [-1, K_e) or offsets that are not those of the lists, bit 1 a row without a member, bit 2 an
 * index outside the volume at an entry with an id, bit 3 a bounded loop ran out, bit 4 a cls >= 32 (such an entry or row is
 * skipped); URSN_CLGRAPH_EDGE_OVERFLOW: more than edge_cap distinct edges exist -- decided by the arguments alone -- and then only
 * *status is defined.  Rows, groups and edges at or beyond cap_rows / cap_groups / edge_out_cap are never written; everything below
 * them is complete whatever the caps are; edge_offsets and group_offsets hold the true counts.  Null, misaligned, out-of-domain and
 * too-small arguments are refused with a message that begins "cluster_graph:" before any launch. */
#define URSN_CLGRAPH_E 6    /* int64 columns of an edge record */
#define URSN_CLGRAPH_I 6    /* int64 columns of a row record */
#define URSN_CLGRAPH_G 12   /* int64 columns of a group record */
#define URSN_CLGRAPH_EV 4   /* int64 columns of an event record */
#define URSN_CLGRAPH_EDGE_OVERFLOW 256 /* bit of *status */

typedef struct ursn_cluster_graph_desc { /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t gap;                          /* 1..3 */
  int64_t m_total;                      /* list entries, < 2^31 */
  int64_t edge_cap;                     /* distinct edges the scratch has room for, [0, 2^30) */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] strictly increasing per event */
  const int32_t* cluster;               /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets;         /* [n+1] */
  const float* value;                   /* [m_total], or null: every charge is 0 */
  const uint8_t* cls;                   /* [K_total] the cluster table's cls, or null: every class mask is 0 */
} ursn_cluster_graph_desc;

typedef struct ursn_cluster_graph_out { /* DEVICE pointers */
  int64_t* rows;                        /* [cap_rows][URSN_CLGRAPH_I] */
  int64_t cap_rows;
  int64_t* groups;                      /* [cap_groups][URSN_CLGRAPH_G] */
  int64_t cap_groups;
  int64_t* group_offsets;               /* [n+1] */
  int64_t* event;                       /* [n][URSN_CLGRAPH_EV] */
  int32_t* group;                       /* [m_total] */
  int64_t* edge_offsets;                /* [cap_rows + 1], or null: no edge list; entries 0 .. min(K_total, cap_rows) are written */
  int64_t* edges;                       /* [edge_out_cap][URSN_CLGRAPH_E], or null: the counts in edge_offsets only */
  int64_t edge_out_cap;
  int32_t* status;                      /* [1] */
} ursn_cluster_graph_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535], m_total outside [0, 2^31), a cap < 0 or edge_cap outside
 * [0, 2^30).  Host logic only. */
size_t ursn_cluster_graph_scratch_bytes(int32_t n, int64_t m_total, int64_t cap_rows, int64_t cap_groups, int64_t edge_cap);
int ursn_cluster_graph(const ursn_cluster_graph_desc* d, const ursn_cluster_graph_out* out, void* scratch, size_t scratch_bytes,
                       void* stream);

/* ---- per-cluster charge profiles along the principal axis (cluster_profile.hip) ---------------------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * The step after the object record: the charge of a cluster segment by segment along its axis (dQ/dx, which end the charge rises
 * towards, empty segments of a broken track, the kink of the trajectory through the segment centroids).  Input: the lists and ids
 * ursn_cluster_features read and the two tables it wrote for them.  uresnet_amd/clusters.py (cluster_profile_numpy) states every
 * field operation by operation; the device gives the same bits.
 *
 * Row r with the object record's n, anchor m, axis, t_lo and length has, in fp64 and one rounded operation at a time,
 *   nb_true = floor(length / step) + 1     nb = min(nb_true, max_bins)     pad = ((double)nb_true * step - length) / 2
 * segments (bins).  A member's bin is b = min(max(floor((((double)t - t_lo) + pad) / step), 0), nb - 1) with t the object record's
 * fp32 projection of the member.  Bins are CSR by global row: bin_offsets[r] .. bin_offsets[r + 1].
 * Bin record, URSN_CLPROF_BI int64:  [0] n   [1] charge = sum of rint((double)value * 2^16) (|value| >= 2^15 or a non-finite value
 *   adds nothing and sets bit 0 of flags; no value list: 0)   [2..4] d = sum (x - m)   [5] flags.
 * Bin record, URSN_CLPROF_BR fp64:   [0..2] c = (double)m + (double)d / (double)n   [3] dqdx = ((double)charge / 2^16) / step;
 *   an empty bin holds +0.0 in all four.
 * Row record, URSN_CLPROF_RI int64:  [0] bins = nb   [1] filled   [2] gaps (maximal runs of empty bins between filled ones)
 *   [3] longest_gap   [4] peak_bin (largest charge, lowest among equals)   [5] h = min(end_bins, nb / 2)   [6] head_n, [7] head_charge
 *   over bins [0, h)   [8] tail_n, [9] tail_charge over bins [nb - h, nb)   [10] direction = sign(tail_charge - head_charge), 0 for
 *   h == 0: a charge-asymmetry sign and nothing more   [11] flags: bit 0 a bin is flagged, bit 1 nb_true > max_bins (truncated).
 * Row record, URSN_CLPROF_RR fp64:   [0] path = length of the polyline through the centroids of the filled bins   [1] min_cos = the
 *   smallest cosine between consecutive polyline segments (1.0 without a pair)   [2] kink_bin = the bin of that pair's middle point
 *   (-1.0 without one)   [3] head_dqdx, [4] tail_dqdx = ((double)charge / 2^16) / ((double)h * step) (0.0 for h == 0)
 *   [5] straightness = length / path (1.0 for path == 0).
 * Bounds with every extent <= 32768 and m_total < 2^31: bin n < 2^31, |d| < 2^46, |charge| <= 2^62, nb <= 65536.
 *
 * Method: per row nb; a one-workgroup scan into bin_offsets; the bins below the total cleared; one thread per list entry adds n,
 * charge and d with 64-bit INTEGER atomic adds at agent scope and ors the flag, nothing else (equal bins of adjacent lanes of a wave
 * are combined first, then a workgroup's runs in a 256-slot LDS table that falls through to direct atomics when full;
 * URSN_CLPROF_WAVE=0: one atomic set per entry; same bits); one thread per bin for the fp64 columns; one thread per row for the row
 * record.  Six launches, enqueues only, never synchronises; the scratch needs no initialisation; every device loop is bounded.
 *
 * Rows considered: below min(table_offsets[n], feat_cap, cap_rows, m_total); rows at or beyond it are never written, and bin_offsets
 * is written for entries 0 .. that count and holds the true counts whatever bin_cap is.  *status is 0, or: bit 0 an id outside its
 * event's rows, offsets that are not those of the lists, an index outside the volume at an entry with an id, or a length that is no
 * object record's; bit 1 a row without a member (such entries and rows are skipped, a skipped row has no bins);
 * URSN_CLPROF_BIN_OVERFLOW: the total exceeds bin_cap -- decided by the arguments alone -- and then only bin_offsets and *status
 * are defined.  Null, misaligned, out-of-domain and too-small arguments are refused with a message that begins "cluster_profile:"
 * before any launch. */
#define URSN_CLPROF_BI 6    /* int64 columns of a bin record */
#define URSN_CLPROF_BR 4    /* fp64 columns of a bin record */
#define URSN_CLPROF_RI 12   /* int64 columns of a row record */
#define URSN_CLPROF_RR 6    /* fp64 columns of a row record */
#define URSN_CLPROF_BIN_OVERFLOW 256 /* bit of *status */

typedef struct ursn_cluster_prof_desc { /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t reserved;                     /* 0 */
  int64_t m_total;                      /* list entries, < 2^31 */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] */
  const float* value;                   /* [m_total], or null: charge = 0 */
  const int32_t* cluster;               /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets;         /* [n+1] as ursn_cluster_voxels wrote it */
  const int64_t* itab;                  /* [feat_cap][URSN_CLFEAT_I] as ursn_cluster_features wrote it for these lists */
  const double* rtab;                   /* [feat_cap][URSN_CLFEAT_R] */
  int64_t feat_cap;                     /* the cap of those tables */
  double step;                          /* finite, [0.5, 4096] */
  int32_t end_bins;                     /* 1..16 */
  int32_t max_bins;                     /* 1..65536 */
} ursn_cluster_prof_desc;

typedef struct ursn_cluster_prof_out {  /* DEVICE pointers */
  int64_t* bin_offsets;                 /* [cap_rows + 1] */
  int64_t* bin_itab;                    /* [bin_cap][URSN_CLPROF_BI] */
  double* bin_rtab;                     /* [bin_cap][URSN_CLPROF_BR] */
  int64_t* row_itab;                    /* [cap_rows][URSN_CLPROF_RI] */
  double* row_rtab;                     /* [cap_rows][URSN_CLPROF_RR] */
  int64_t cap_rows;
  int64_t bin_cap;                      /* [0, 2^31) */
  int32_t* status;                      /* [1] */
} ursn_cluster_prof_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535], m_total outside [0, 2^31), cap_rows < 0 or bin_cap
 * outside [0, 2^31).  Host logic only. */
size_t ursn_cluster_profile_scratch_bytes(int32_t n, int64_t m_total, int64_t cap_rows, int64_t bin_cap);
int ursn_cluster_profile(const ursn_cluster_prof_desc* d, const ursn_cluster_prof_out* out, void* scratch, size_t scratch_bytes,
                         void* stream);

/* ---- cluster chains: broken track fragments joined end to end (cluster_chain.hip) -----------------------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.  (The section stands here, before the last one, because
 * existing tests pin that one as the header's end; nothing before or after it moved.)
 * A connected component is not a particle: a dead wire or a few lost voxels cut one track into collinear fragments.  This call
 * joins them: end points of different rows that face each other across a gap, with both axes and the gap vector collinear, are
 * joined when the choice is mutual; rows linked by joins form a CHAIN, and the chains come back as a second clustering of the same
 * lists in the (cluster, table_offsets, first / size / cls) format of ursn_cluster_voxels, so every call that takes a clustering
 * runs on the merged objects unchanged.  Input: the lists and ids ursn_cluster_features read, the two tables it wrote for them,
 * optionally the cluster table's cls.  uresnet_amd/clusters.py (cluster_chains_numpy) states every field operation by operation;
 * the device gives the same bits.
 *
 * A global row r is ELIGIBLE when its object record has n >= min_size and end_lo != end_hi and, with class_mask != 0, bit cls[r] of
 * class_mask is set.  An eligible row has two END POINTS, at the list positions end_lo and end_hi, with the KEY 2 r + side (side 0 =
 * end_lo) and the DIRECTION u = +axis at the lo end, -axis at the hi end (it points from the end into the row).  Coordinates x[0..2]
 * are the row-major coordinates of index[j] in `spatial` (2-D: x[2] = 0).  A CANDIDATE is a pair of end points p < q (by key) of one
 * event and of DIFFERENT rows whose coordinates differ by at most max_gap on every axis and, with same_class, whose rows have equal
 * cls.  It is evaluated once, p the lower key, every operation rounded on its own:
 *   d = x(q) - x(p)     dist2 = d . d  (1 .. 3 * 31^2 = 2883)     s = sqrt((double)dist2)
 *   c_ax = -((u_p[0] * u_q[0] + u_p[1] * u_q[1]) + u_p[2] * u_q[2])
 *   c_lo = (-((u_p[0] * d0 + u_p[1] * d1) + u_p[2] * d2)) / s        c_hi = ((u_q[0] * d0 + u_q[1] * d1) + u_q[2] * d2) / s
 * and ACCEPTED when c_ax >= min_cos && c_lo >= min_cos && c_hi >= min_cos (a NaN rejects).  Every end point counts its accepted
 * candidates and picks as BEST the one smallest in (dist2, partner key); {p, q} is a JOIN when each is the other's best: an end
 * point is in at most one join, a row in at most two.  Rows linked by joins are unioned; a CHAIN is a component, numbered per event
 * by its lowest row: chain_offsets[n + 1].  Every row below the row count is in exactly one chain.
 * merged[j]: the event-local chain of cluster[j]'s row, -1 where cluster[j] is -1.  Chain table: first = the lowest event-local
 * list position of a member, size = members, cls = cls of the lowest row (0 without cls).
 * Chain record, URSN_CLCHAIN_CI int64:
 *   [0] rows   [1] joins   [2] n, [3] charge   summed over the object records   [4..6] lo, [7..9] hi   the union of their boxes
 *   [10] first_row  event-local   [11] end_a, [12] end_b   list positions (the walk)   [13] gap2_sum, [14] gap2_max   over the joins'
 *   dist2   [15] class mask of the rows (0 without cls) | flags << 32; flag bit 0: a ring (no free end); flag bit 1: a member row
 *   whose object record has flags != 0
 * Chain record, URSN_CLCHAIN_CR fp64:  [0] path   [1] gaps   [2] span   [3] straightness   [4] min_cos, by THE WALK: START is the
 *   chain's free end point (an end of a member row that is in no join; a row that is not eligible has two) with the lowest key, a
 *   ring starts at the lo side of first_row; end_a is START's position; enter the start row at that side, then `rows` times:
 *   path = path + length[row]; leave at the other side; if that side is in a join and fewer than `joins` joins were taken:
 *   g = sqrt((double)dist2), path = path + g, gaps = gaps + g, min_cos takes the join's c_ax if it is the first or strictly smaller,
 *   enter the partner row at the partner's side.  end_b is the position of the end at which the walk leaves its last row;
 *   span = sqrt((double)(squared distance between the coordinates of end_a and end_b)); straightness = span / path, +0.0 when
 *   path == 0.0; min_cos and gaps are +0.0 without joins.
 * Join record, CSR by event (join_offsets[n + 1]), ascending key_a.  URSN_CLCHAIN_JI int64: [0] key_a < [1] key_b (event-local
 *   keys)   [2] dist2   [3] pos_a, [4] pos_b   list positions   [5] chain (event-local).  URSN_CLCHAIN_JR fp64: [0] c_ax   [1] c_lo
 *   [2] c_hi   [3] gap = sqrt((double)dist2).
 * Per row: row_chain int32; row_join int32 [2] = the partner's event-local key at the lo / hi side, -1 for none; row_candidates
 * int32 [2].  Event record, URSN_CLCHAIN_EV int64: [0] chains   [1] joins   [2] joined (chains with rows >= 2)   [3] longest = the
 * chain largest in (rows, n), the lowest id among equals; -1 without chains.
 * What it does not decide: whether a joined pair is one particle stays the consumer's judgement; the cosines and the gap are there
 * to cut on.
 *
 * Bounds with every extent <= 32768, m_total < 2^30 and K rows: at most K joins (an end point is in at most one, a join takes two),
 * so no table of this call can overflow; the rows of a chain are distinct rows of one event, so n < 2^31 and |charge| <= 2^62;
 * gap2_sum <= 2883 K.  The packed words fit: dist2 << 32 | key with dist2 <= 2883 and key < 2^31 (m_total is bounded by 2^30 so that
 * every key 2 r + side is an int32); rows << 32 | n with rows < 2^30 and n < 2^31, below 2^63.
 *
 * Method: twelve launches (cluster_chain.hip lists them).  The search does not walk list rows -- the gaps are up to 31 voxels and
 * there are at most 2 K end points: the end positions of the eligible rows are marked, counted per tile of 64 entries, scanned by one
 * workgroup and compacted in list order, so the compact array is sorted by event << 32 | index; the end points of plane x0 + d0
 * with x1 within max_gap are one contiguous range of it (a 2-D list runs as (s0, s1, 1)), found by a lower-bound binary search
 * (<= 32 halvings) and left at the range's last index, then filtered on x2, row and class.  One wave64 per end point, one lane per
 * plane (2 max_gap + 1 <= 63 lanes), a wave reduction of ONE packed minimum dist2 << 32 | key and of the accepted count: the wave
 * owns its end point, no atomics in the search (URSN_CLCHAIN_WAVE=0: one thread per end point takes its planes one after another;
 * same bits).  A mutual test per end point; a union-find over rows with 32-bit atomicMin to the lower root; one-workgroup scans for
 * the chain numbers and the join list; per row 64-bit INTEGER atomic adds / min / max / ors at agent scope onto its chain; per entry
 * merged and an integer atomic minimum for first; one thread per chain walks it and computes every fp64 value in the order above
 * under contract(off); a packed 64-bit atomic maximum and one minimum find the longest.  No float atomics.  Enqueues only, never
 * synchronises; the scratch needs no initialisation; every device loop is bounded; the same arguments give the same bits.
 *
 * Rows considered: below min(table_offsets[n], feat_cap, m_total).  *status is 0, or: bit 0 an id outside [-1, K_e) or offsets that
 * are not those of the lists, bit 1 a row without a member, bit 2 an index outside the volume at an entry with an id, bit 3 a bounded
 * loop ran out, bit 4 a cls >= 32, bit 5 an end position of an otherwise eligible row that is not a member of it, bit 6
 * table_offsets[n] > feat_cap (such a row is not eligible and stays a chain of one, such an entry gets merged = -1; every entry with
 * an id and every row is checked, and the bits are the same whenever the arguments are).  Chains, joins and rows at or beyond
 * cap_chains / cap_joins / cap_rows are never written; everything below them is complete whatever the caps are; chain_offsets,
 * join_offsets and the event records hold the true counts.  m_total = 0 or no clusters still writes *status, the offsets and the
 * event records.  Null, misaligned, out-of-domain and too-small arguments are refused with a message that begins "cluster_chains:"
 * before any launch. */
#define URSN_CLCHAIN_CI 16   /* int64 columns of a chain record */
#define URSN_CLCHAIN_CR 5    /* fp64 columns of a chain record */
#define URSN_CLCHAIN_JI 6    /* int64 columns of a join record */
#define URSN_CLCHAIN_JR 4    /* fp64 columns of a join record */
#define URSN_CLCHAIN_EV 4    /* int64 columns of an event record */

typedef struct ursn_cluster_chain_desc { /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t max_gap;                      /* 1..31 */
  int64_t m_total;                      /* list entries, < 2^30 */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] strictly increasing per event */
  const int32_t* cluster;               /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets;         /* [n+1] as ursn_cluster_voxels wrote it */
  const int64_t* itab;                  /* [feat_cap][URSN_CLFEAT_I] as ursn_cluster_features wrote it for these lists */
  const double* rtab;                   /* [feat_cap][URSN_CLFEAT_R] */
  int64_t feat_cap;                     /* the cap of those tables */
  const uint8_t* cls;                   /* [K_total] the cluster table's cls, or null: every class mask is 0 */
  double min_cos;                       /* [0, 1] */
  int32_t min_size;                     /* >= 1 */
  uint32_t class_mask;                  /* 0: rows of every class are eligible; else bit cls[r] decides, and cls must be given */
  int32_t same_class;                   /* 0 | 1: only rows of equal cls are joined, and cls must be given */
  int32_t reserved;                     /* 0 */
} ursn_cluster_chain_desc;

typedef struct ursn_cluster_chain_out { /* DEVICE pointers */
  int32_t* merged;                      /* [m_total] */
  int64_t* chain_offsets;               /* [n+1] */
  int32_t* first;                       /* [cap_chains] the chain table, typed as ursn_cluster_out's */
  int32_t* size;                        /* [cap_chains] */
  uint8_t* cls;                         /* [cap_chains] */
  int64_t* chain_itab;                  /* [cap_chains][URSN_CLCHAIN_CI] */
  double* chain_rtab;                   /* [cap_chains][URSN_CLCHAIN_CR] */
  int64_t cap_chains;
  int64_t* join_offsets;                /* [n+1] */
  int64_t* join_itab;                   /* [cap_joins][URSN_CLCHAIN_JI] */
  double* join_rtab;                    /* [cap_joins][URSN_CLCHAIN_JR] */
  int64_t cap_joins;
  int32_t* row_chain;                   /* [cap_rows] */
  int32_t* row_join;                    /* [cap_rows][2] */
  int32_t* row_candidates;              /* [cap_rows][2] */
  int64_t cap_rows;
  int64_t* event;                       /* [n][URSN_CLCHAIN_EV] */
  int32_t* status;                      /* [1] */
} ursn_cluster_chain_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535] or m_total outside [0, 2^30).  Host logic only. */
size_t ursn_cluster_chains_scratch_bytes(int32_t n, int64_t m_total);
int ursn_cluster_chains(const ursn_cluster_chain_desc* d, const ursn_cluster_chain_out* out, void* scratch, size_t scratch_bytes,
                        void* stream);

/* ---- cluster cones: shower fragments gathered to their primary (cluster_cone.hip) ------------------------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.  (The section stands here, before the last one, for the reason
 * the cluster-chains section gives.)
 * An electromagnetic shower is one narrow start fragment with tens of small, disconnected fragments downstream of it: no axis to
 * speak of, no end that faces anything, up to a radiation length away.  This call gathers them: every fragment (CHILD) looks for the
 * end point (APEX) of a larger row inside whose cone it lies and LINKS to the nearest; the links form a forest, a SHOWER is a tree,
 * and the showers come back as one more clustering of the same lists in the (cluster, table_offsets, first / size / cls) format of
 * ursn_cluster_voxels, so every call that takes a clustering runs on them unchanged.  Input: as ursn_cluster_chains.
 * uresnet_amd/clusters.py (cluster_cones_numpy) states every field operation by operation; the device gives the same bits.
 *
 * A global row C is CHILD-eligible when its object record has n >= min_size and, with class_mask != 0, bit cls[C] of class_mask is
 * set.  A global row P is PARENT-eligible when n >= seed_size and end_lo != end_hi under the same class condition; it has two
 * APEXES, at the list positions end_lo and end_hi, with the KEY 2 P + side (side 0 = end_lo) and the DIRECTION u = +axis at the lo
 * end, -axis at the hi end (from the end into the row): the chains' end points.  A child is represented by its anchor m (itab[11..13]
 * of its object record, the centroid rounded to a voxel).  Coordinates x[0..2] are the row-major coordinates of index[j] in `spatial`
 * (2-D: x[2] = 0).  P OUTRANKS C when n_P > n_C, or n_P == n_C and P < C: a strict total order, so links never form a cycle.
 * A CANDIDATE is a child C and an apex (P, side) of different rows of one event, P outranking C and, with same_class, of equal cls,
 * with d = m_C - x(apex) as integers, every fp64 operation rounded on its own:
 *   |d_a| <= reach on every axis   and   1 <= dist2 = d . d <= reach^2          s = sqrt((double)dist2)
 *   t = (u[0] * d0 + u[1] * d1) + u[2] * d2          c_cone = t / s
 *   c_ax = fabs((u[0] * a0 + u[1] * a1) + u[2] * a2)   a = axis of C; formed only when C is itself PARENT-eligible
 * and ACCEPTED when c_cone >= min_cos and, where c_ax is formed, c_ax >= min_cos (a NaN rejects).  Every child counts its accepted
 * candidates and takes as its PARENT apex the one smallest in (dist2, apex key): a LINK.  No mutual test: a parent may have many
 * children, a row at most one parent.  The PRIMARY of a shower is its tree's root; a row's depth is its number of links to the root.
 * Showers are numbered per event by their lowest row: shower_offsets[n + 1].  Every row below the row count is in exactly one shower.
 * merged[j]: the event-local shower of cluster[j]'s row, -1 where cluster[j] is -1.  Shower table: first = the lowest event-local
 * list position of a member, size = members, cls = cls of the PRIMARY (0 without cls).
 * Shower record, URSN_CLCONE_SI int64:
 *   [0] rows   [1] n, [2] charge   summed over the object records   [3..5] lo, [6..8] hi   the union of their boxes
 *   [9] first_row, [10] primary   event-local rows   [11] start = the list position of the primary's apex on the START side: the side
 *   with the larger summed n of its DIRECT children, among equals the side with more direct children, then side 0 (a primary that
 *   is not parent-eligible: end_lo)   [12] depth   the largest of a row   [13] dist2_max   over the links   [14] primary_n
 *   [15] class mask of the rows (0 without cls) | flags << 32; flag bit 0: the primary has direct children at both apexes; flag bit
 *   1: a member row whose object record has flags != 0
 * Shower record, URSN_CLCONE_SR fp64:  [0] primary_fraction = (double)primary_n / (double)n   [1] min_cos = the smallest c_cone,
 *   [2] t_max = the largest t over the links, both +0.0 without links   [3] r_max = sqrt((double)dist2_max).
 * Link record, CSR by event (link_offsets[n + 1]), ascending child row.  URSN_CLCONE_LI int64: [0] child (event-local row)
 *   [1] apex (event-local key)   [2] dist2   [3] pos = list position of the apex   [4] shower (event-local)   [5] depth of the child.
 *   URSN_CLCONE_LR fp64: [0] c_cone   [1] t   [2] r = s   [3] c_ax (+0.0 where it was not formed).
 * Per row: row_shower int32; row_parent int32 = the event-local apex key, -1 for none; row_candidates int32; row_children int32 [2]
 * = direct children at the lo / hi apex; row_depth int32.  Event record, URSN_CLCONE_EV int64: [0] showers   [1] links   [2] grouped
 * (showers with rows >= 2)   [3] largest = the shower largest in (rows, n), the lowest id among equals; -1 without showers.
 * What it does not decide: whether a linked fragment belongs to the shower stays the consumer's judgement; c_cone, t and r are there
 * to cut on.
 *
 * Bounds with every extent <= 32768, m_total < 2^30 and K rows: at most K links (a row has at most one parent), so no table of
 * this call can overflow; dist2 <= 127^2 = 16129; the packed word dist2 << 32 | apex key needs keys below 2^31, hence m_total < 2^30;
 * the rows of a shower are distinct rows of one event, so n < 2^31 and |charge| <= 2^62; rows << 32 | n is below 2^63.
 *
 * Method: twelve launches (cluster_cone.hip lists them).  The apexes of the parent-eligible rows are marked, counted per tile of
 * 64 entries, scanned by one workgroup and compacted in list order, so the compact array is sorted by event << 32 | index; for a
 * child with anchor (m0, m1, m2) the apexes of plane m0 + d0 with x1 within reach are one contiguous range of it (a 2-D list runs as
 * (s0, s1, 1)), found by a lower-bound binary search and filtered on x2, row, rank, class and the Euclidean bound.  One wave64 per
 * child row, the lanes striding the 2 reach + 1 <= 255 planes (up to four trips), then a butterfly reduction of ONE packed minimum
 * dist2 << 32 | apex key and of the accepted count: the wave owns its child, no atomics in the search (URSN_CLCONE_WAVE=0: one
 * thread per child row takes its planes one after another; same bits).  Per row a walk up the parents for the root and the depth
 * (rank strictly rises; capped at the row count) and an integer atomic minimum for the tree's lowest row; one-workgroup scans for
 * the shower numbers and the link list; per row 64-bit INTEGER atomic adds / min / max / ors at agent scope onto its shower and its
 * parent's counters (min_cos and t_max are strictly positive doubles: integer min / max on their bit patterns); per entry merged and
 * an integer atomic minimum for first; one thread per shower and per link for the fp64 columns, under contract(off).  No float
 * atomics.  Enqueues only, never synchronises; the scratch needs no initialisation; every device loop is bounded; the same arguments
 * give the same bits.
 *
 * Rows considered: below min(table_offsets[n], feat_cap, m_total).  *status is 0, or: bit 0 an id outside [-1, K_e) or offsets that
 * are not those of the lists, bit 1 a row without a member, bit 2 an index outside the volume at an entry with an id, bit 3 a bounded
 * loop ran out, bit 4 a cls >= 32, bit 5 an end position of an otherwise parent-eligible row that is not a member of it or an anchor
 * outside the volume, bit 6 table_offsets[n] > feat_cap (such a row takes no part and stays a shower of one, such an entry gets
 * merged = -1; every entry with an id and every row is checked, and the bits are the same whenever the arguments are).  Showers,
 * links and rows at or beyond cap_showers / cap_links / cap_rows are never written; everything below them is complete whatever the
 * caps are; shower_offsets, link_offsets and the event records hold the true counts.  m_total = 0 or no clusters still writes
 * *status, the offsets and the event records.  Null, misaligned, out-of-domain and too-small arguments are refused with a message
 * that begins "cluster_cones:" before any launch. */
#define URSN_CLCONE_SI 16   /* int64 columns of a shower record */
#define URSN_CLCONE_SR 4    /* fp64 columns of a shower record */
#define URSN_CLCONE_LI 6    /* int64 columns of a link record */
#define URSN_CLCONE_LR 4    /* fp64 columns of a link record */
#define URSN_CLCONE_EV 4    /* int64 columns of an event record */

typedef struct ursn_cluster_cone_desc { /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t reach;                        /* 1..127 */
  int64_t m_total;                      /* list entries, < 2^30 */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] strictly increasing per event */
  const int32_t* cluster;               /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets;         /* [n+1] as ursn_cluster_voxels wrote it */
  const int64_t* itab;                  /* [feat_cap][URSN_CLFEAT_I] as ursn_cluster_features wrote it for these lists */
  const double* rtab;                   /* [feat_cap][URSN_CLFEAT_R] */
  int64_t feat_cap;                     /* the cap of those tables */
  const uint8_t* cls;                   /* [K_total] the cluster table's cls, or null: every class mask is 0 */
  double min_cos;                       /* (0, 1] */
  int32_t min_size;                     /* >= 1: fewest members of a child */
  uint32_t class_mask;                  /* 0: rows of every class take part; else bit cls[r] decides, and cls must be given */
  int32_t same_class;                   /* 0 | 1: only rows of equal cls are linked, and cls must be given */
  int32_t seed_size;                    /* >= 2: fewest members of a parent */
} ursn_cluster_cone_desc;

typedef struct ursn_cluster_cone_out { /* DEVICE pointers */
  int32_t* merged;                      /* [m_total] */
  int64_t* shower_offsets;              /* [n+1] */
  int32_t* first;                       /* [cap_showers] the shower table, typed as ursn_cluster_out's */
  int32_t* size;                        /* [cap_showers] */
  uint8_t* cls;                         /* [cap_showers] */
  int64_t* shower_itab;                 /* [cap_showers][URSN_CLCONE_SI] */
  double* shower_rtab;                  /* [cap_showers][URSN_CLCONE_SR] */
  int64_t cap_showers;
  int64_t* link_offsets;                /* [n+1] */
  int64_t* link_itab;                   /* [cap_links][URSN_CLCONE_LI] */
  double* link_rtab;                    /* [cap_links][URSN_CLCONE_LR] */
  int64_t cap_links;
  int32_t* row_shower;                  /* [cap_rows] */
  int32_t* row_parent;                  /* [cap_rows] */
  int32_t* row_candidates;              /* [cap_rows] */
  int32_t* row_children;                /* [cap_rows][2] */
  int32_t* row_depth;                   /* [cap_rows] */
  int64_t cap_rows;
  int64_t* event;                       /* [n][URSN_CLCONE_EV] */
  int32_t* status;                      /* [1] */
} ursn_cluster_cone_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535] or m_total outside [0, 2^30).  Host logic only. */
size_t ursn_cluster_cones_scratch_bytes(int32_t n, int64_t m_total);
int ursn_cluster_cones(const ursn_cluster_cone_desc* d, const ursn_cluster_cone_out* out, void* scratch, size_t scratch_bytes,
                       void* stream);

/* ---- cluster splits: a component of several particles cut at its junctions and kinks (cluster_split.hip) ---------------------------
 * Every call above takes a connected component for an object.  The chain and cone calls repair one way that fails (one particle in
 * several components); this call repairs the other: several particles in ONE component -- the prongs of a vertex, two tracks that
 * cross, a track with a hard kink.  It returns one more clustering of the same lists, in the format ursn_cluster_voxels writes
 * (split ids, piece_offsets, first / size / cls), so every call that takes a clustering runs on the pieces unchanged; the intended
 * order is components -> split -> chains -> cones.  uresnet_amd/clusters.py (cluster_split_numpy) is the definition, operation by
 * operation; this call gives its bits.
 *
 * ADJACENT: two different entries of one event whose coordinates differ by at most 1 on every axis (full adjacency, whatever
 * connectivity made the clustering; decided on coordinates, never on linear indices; cells outside the volume are empty; a 2-D list
 * has x2 = 0).  ELIGIBLE: a global row r with size[r] >= min_size and, with class_mask, bit cls[r] of it set.
 *
 * ARMS, for every member j of an eligible row R.  BALL(j) = the members of R within Chebyshev distance radius of x(j); REACH(j) = the
 * entries of BALL(j) joined to j by a path of adjacent entries inside BALL(j); SHELL(j) = the entries of REACH(j) at distance exactly
 * radius; the arms are the connected components of SHELL(j) under adjacency among shell entries, arms(j) = min(their number, 15).  An
 * end sees 1 arm, a body 2, a junction 3 or more; a stub shorter than radius makes none.  KINK (only with exactly 2 arms and
 * kink_cos < 1): s_a = the integer sum of x(q) - x(j) over arm a, dot = s_1 . s_2, q_a = s_a . s_a, and with both q_a > 0
 * c = (double)dot / (sqrt((double)q_1) * sqrt((double)q_2)); KINK iff c > kink_cos.  j is CUT when arms(j) >= 3 or KINK.
 *
 * PIECES: among the entries of eligible rows, adjacent entries of one row with equal cut status are joined; uncut components are
 * pieces of kind 1, cut components are JUNCTIONS; a row that is not eligible is one piece of kind 0, whole, connected or not (an
 * eligible row that is itself disconnected falls into its components: split BEFORE chaining).  ATTACHMENT, rounds t = 1 .. grow: a
 * cut entry without a piece looks at its adjacent entries of the same row that are uncut or were attached in a round before t and
 * takes the piece of the one at the lowest list position; a round reads only what earlier rounds wrote.  What a junction still holds
 * after the last round is one piece of kind 2.  Pieces are numbered per event by ascending KEY (kinds 0 and 1: the lowest list
 * position of the original members; kind 2: the lowest position of the junction's entries before attachment), junctions per event
 * by their lowest position.  With attachment `first` need not ascend with the piece id; no call of this header relies on that.
 * A CONTACT is an ordered pair (cut entry, adjacent uncut entry of its row), taken before attachment.
 *
 * mark[j] = arms | cut << 4 | kink << 5 | attached << 6, 0 where the entry was not evaluated.
 * Piece record, URSN_CLSPLIT_PI int64: [0] row (event-local)   [1] n final members   [2] attached (of them)   [3] kind
 *   [4] key (a list position)   [5] contacts whose uncut entry is an original member   [6] junction_lo, [7] junction_hi the smallest
 *   / largest event-local junction of those contacts, -1 for none (a piece of kind 2: contacts 0 and its own junction in both).
 * Junction record, URSN_CLSPLIT_JI int64: [0] row   [1] entries   [2] attached   [3] arms_max   [4] kink entries   [5..7] coordinate
 *   sums   [8..10] box lo   [11..13] box hi   [14] first position   [15] contacts   [16] piece_lo, [17] piece_hi the smallest / largest
 *   event-local piece among its contacts' uncut entries, -1 for none.  URSN_CLSPLIT_JR fp64: [0..2] centroid = (double)sum /
 *   (double)entries -- the vertex position that ursn_cluster_vertices cannot see inside one component.
 * Per row, URSN_CLSPLIT_ROW int32: pieces, junctions, cut entries.  Event record, URSN_CLSPLIT_EV int64: [0] pieces   [1] junctions
 *   [2] rows with a junction   [3] cut entries.
 *
 * Method (cluster_split.hip lists the launches).  The hot pass is the arms count: the entries of eligible rows are compacted in list
 * order.  The list row (x0 - radius + a, x1 - radius + b) of an entry's ball is found by ONE lower-bound binary search confined to
 * the event's range (<= 32 halvings); at most 7 consecutive entries are read and a 7-bit mask of the members of R kept; the masks
 * make the ball's bitmap, seven 64-bit words, one per x2 and bit 8 a + b inside.  REACH is an iterated dilation of the centre bit
 * inside the bitmap (shifts by 1, 8 and a word), the arms the same flood from successive lowest seeds inside the shell mask.  The
 * default (and URSN_CLSPLIT_WAVE=0) is the plain form, one thread per entry, its seven words in registers; URSN_CLSPLIT_WAVE=1 is
 * the wave form, one wave64 per entry, lane 8 a + b < 56 owns one list row and seven ballots make the words (same bits; slower as
 * measured, because its flood is uniform and runs on the scalar unit).  Then a union-find over the equal-status adjacency with 32-bit atomicMin to the lower position, `grow` attachment
 * launches whose round stamp only its owner writes, ballot counts per tile of 64 entries and one-workgroup scans for the two
 * numberings, and 64-bit INTEGER atomic adds / min / max at agent scope for the records; each centroid is one thread's three
 * divisions under contract(off).  No float atomics.  Enqueues only, never synchronises; the scratch needs no initialisation; every
 * device loop is bounded; the same arguments give the same bits.
 *
 * *status is 0, or: bit 0 an id outside [-1, K_e), offsets that are not those of the lists or table_offsets[n] > m_total, bit 1 a
 * list that does not increase strictly inside an event, bit 2 an index outside the volume at an entry with an id, bit 3 a bounded
 * loop ran out, bit 4 a cls >= 32 (such an entry or row takes no part: split = -1, mark = 0; every entry and row is checked and the
 * bits are the same whenever the arguments are).  Pieces, junctions and rows at or beyond cap_pieces / cap_junctions / cap_rows are
 * never written; everything below them is complete whatever the caps are; piece_offsets, junction_offsets and the event records
 * hold the true counts.  m_total = 0 still writes *status, the offsets and the event records.  Null, misaligned, out-of-domain and
 * too-small arguments are refused with a message that begins "cluster_split:" before any launch. */
#define URSN_CLSPLIT_PI 8    /* int64 columns of a piece record */
#define URSN_CLSPLIT_JI 18   /* int64 columns of a junction record */
#define URSN_CLSPLIT_JR 3    /* fp64 columns of a junction record */
#define URSN_CLSPLIT_ROW 3   /* int32 columns per row */
#define URSN_CLSPLIT_EV 4    /* int64 columns of an event record */

typedef struct ursn_cluster_split_desc { /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t radius;                       /* 1..3 */
  int64_t m_total;                      /* list entries, < 2^30 */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] strictly increasing per event */
  const int32_t* cluster;               /* [m_total] event-local ids, -1 for none */
  const int64_t* table_offsets;         /* [n+1] */
  const int32_t* size;                  /* [K_total] the cluster table's size */
  const uint8_t* cls;                   /* [K_total] the cluster table's cls, or null: every cls written is 0 */
  double kink_cos;                      /* [-1, 1]; >= 1: no kinks */
  int32_t min_size;                     /* >= 1 */
  uint32_t class_mask;                  /* 0: rows of every class are eligible; else bit cls[r] decides, and cls must be given */
  int32_t grow;                         /* 0..8 attachment rounds */
  int32_t reserved;                     /* 0 */
} ursn_cluster_split_desc;

typedef struct ursn_cluster_split_out { /* DEVICE pointers */
  int32_t* split;                       /* [m_total] */
  uint8_t* mark;                        /* [m_total] */
  int64_t* piece_offsets;               /* [n+1] */
  int32_t* first;                       /* [cap_pieces] the piece table, typed as ursn_cluster_out's */
  int32_t* size;                        /* [cap_pieces] */
  uint8_t* cls;                         /* [cap_pieces] */
  int64_t* piece_itab;                  /* [cap_pieces][URSN_CLSPLIT_PI] */
  int64_t cap_pieces;
  int64_t* junction_offsets;            /* [n+1] */
  int64_t* junction_itab;               /* [cap_junctions][URSN_CLSPLIT_JI] */
  double* junction_rtab;                /* [cap_junctions][URSN_CLSPLIT_JR] */
  int64_t cap_junctions;
  int32_t* rows;                        /* [cap_rows][URSN_CLSPLIT_ROW] */
  int64_t cap_rows;
  int64_t* event;                       /* [n][URSN_CLSPLIT_EV] */
  int32_t* status;                      /* [1] */
} ursn_cluster_split_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535] or m_total outside [0, 2^30).  Host logic only. */
size_t ursn_cluster_split_scratch_bytes(int32_t n, int64_t m_total);
int ursn_cluster_split(const ursn_cluster_split_desc* d, const ursn_cluster_split_out* out, void* scratch, size_t scratch_bytes,
                       void* stream);

/* ---- vertex candidates: where the end points of the object records meet (cluster_vertex.hip) ----------------------------------------
 * Appended functions and two structs only: URSN_ABI_VERSION stays 9.
 * The step from objects to interactions: which ends meet at one point, how many objects leave it and at what angles, which objects
 * pass it with their body (a T-junction), and which vertex an object starts and stops at.  Input: the lists and ids
 * ursn_cluster_features read, the two tables it wrote for them, optionally the cluster table's cls.  uresnet_amd/clusters.py
 * (cluster_vertices_numpy) states every field operation by operation; the device gives the same bits.
 *
 * A global row r is ELIGIBLE when its object record has n >= min_size and, with class_mask != 0, bit cls[r] of class_mask is set.  An
 * eligible row has END POINTS at the list positions end_lo and end_hi of its object record (one when the two are equal), with the KEY
 * 2 r + side (side 0 = end_lo) and the DIRECTION u = +axis at the lo end, -axis at the hi end (it points from the end into the row).
 * Coordinates x[0..2] are the row-major coordinates of index[j] in `spatial` (2-D: x[2] = 0); two entries are IN REACH when their
 * coordinates differ by at most `radius` on every axis (decided on coordinates: never across a row end, a plane end or an event
 * boundary).  Two end points of one event and of DIFFERENT rows in reach of each other are linked; a VERTEX is a connected component
 * of end points under links, numbered per event in the order of its lowest key: vertex_offsets[n + 1].
 * For every end point p of vertex v and every entry j of the same event with an id in reach of p (j = p included), the pair (p, j)
 * counts towards the INCIDENCE (v, row of j).  Incidence record, URSN_CLVTX_IN int64, CSR by global vertex (inc_offsets[v] ..
 * inc_offsets[v + 1], ascending row):
 *   [0] row   event-local      [1] kind   bit 0 / bit 1: set by the pair (p, p) alone according to p's side, so the set of the row's
 *   own ends inside v; 0 = the row passes v with its body, 3 = both of its ends are in v      [2] near   the number of such pairs
 *   [3] dist2, [4] pos   the squared Euclidean distance and the list position of j of the pair smallest in (dist2, position of j)
 * Vertex record, URSN_CLVTX_VI int64:
 *   [0] ends   [1] rows = incidences   [2] bodies = incidences of kind 0   [3] near summed over the incidences
 *   [4] n, [5] charge   the object records' n and fixed-point charge summed over the incident rows
 *   [6..8] s = the sum of the end-point coordinates   [9..11] lo, [12..14] hi   their box   [15] first_pos = the list position of the
 *   lowest-key end point   [16] class mask of the incident rows (0 without cls) | flags << 32; flag bit 0: more than 16 ends, the
 *   cosines use the first 16; flag bit 1: an incident row with length == 0
 * Vertex record, URSN_CLVTX_VR fp64:
 *   [0..2] c = (double)s / (double)ends   [3] min_cos, [4] max_cos over the pairs i < k of the first min(ends, 16) end directions in
 *   ascending key order, cos = (u_i[0] * u_k[0] + u_i[1] * u_k[1]) + u_i[2] * u_k[2]; both +0.0 with fewer than two ends
 * The record does not decide what the vertex is: two ends with min_cos near -1 and no body are what a broken track looks like, and
 * whether it is one is the consumer's judgement.
 * Per row: row_vertex int32 [2] = the event-local vertex of the lo and the hi end; -1, -1 for a row that is not eligible; both equal
 * for a single end point.  Event record, URSN_CLVTX_EV int64: [0] vertices   [1] junctions (ends >= 2 or bodies >= 1)   [2] free (the
 * others)   [3] primary = the vertex largest in (rows, n), the lowest id among equals; -1 without a vertex.
 *
 * Bounds with every extent <= 32768, m_total < 2^30 and K rows: a vertex has at most 2 K end points with at most 7^3 = 343 entries in
 * reach each, so near < 2 K * 343 < 2^41; the incident rows of a vertex are distinct rows of one event, so n < 2^31 and
 * |charge| <= 2^62; |s| < 2^15 * 2^32 = 2^47; dist2 <= 27.  The packed words fit: vertex << 32 | row with vertex < 2 K < 2^31 and
 * row < 2^30; dist2 << 32 | position with position < 2^30; rows << 32 | n with rows < 2^30 and n < 2^31, below 2^63.  m_total is
 * bounded by 2^30, not 2^31, so that every key 2 r + side is an int32.
 *
 * Method: twelve launches (cluster_vertex.hip lists them).  The walk from an end point visits the (2 radius + 1)^2 rows of the volume
 * around it, one lower-bound binary search (<= 32 halvings) and at most 2 radius + 1 consecutive entries each, no dense map: one
 * wave64 per end point, one lane per row.  Links are a union-find over the keys with 32-bit atomicMin to the lower root; one
 * workgroup scans the root flags, so a vertex's number is the count of roots before its own.  Incidences are counted in an
 * open-addressing table in the scratch, a power of two >= 2 inc_cap + 2 slots keyed vertex << 32 | row: 64-bit compare-and-swap
 * claims, 64-bit INTEGER atomic adds and ors at agent scope, ONE packed 64-bit atomic minimum for (dist2, pos); equal keys of adjacent
 * lanes are combined first, then a workgroup's runs in a 256-slot LDS table that falls through to direct insertions when full
 * (URSN_CLVTX_WAVE=0: one thread per end point, one insertion per pair; same bits).  A slot pass spreads each incidence onto its
 * vertex; scan, drop, rank by row give the list; one thread per vertex computes every fp64 value in the order above under
 * contract(off); a packed 64-bit atomic maximum and one minimum find the primary.  No float atomics.  Enqueues only, never
 * synchronises; the scratch needs no initialisation; every device loop is bounded; the same arguments give the same bits.
 *
 * Rows considered: below min(table_offsets[n], feat_cap, m_total).  *status is 0, or: bit 0 an id outside [-1, K_e) or offsets that
 * are not those of the lists, bit 1 a row without a member, bit 2 an index outside the volume at an entry with an id, bit 3 a bounded loop
 * ran out, bit 4 a cls >= 32, bit 5 an end position that is not a member of its row, bit 6 table_offsets[n] > feat_cap (such an entry
 * or row is skipped; every entry with an id and every row is checked, whether or not a walk meets it, and the bits are the same
 * whenever the arguments are); URSN_CLVTX_INC_OVERFLOW: more than inc_cap distinct incidences exist -- decided by the arguments alone -- and
 * then only vertex_offsets and *status are defined and nothing else is written.  Vertices, incidences and rows at or beyond
 * cap_vertices / inc_out_cap / cap_rows are never written; everything below them is complete whatever the caps are; vertex_offsets
 * and inc_offsets (entries 0 .. min(V, cap_vertices)) hold the true counts.  m_total = 0 or no clusters still writes *status, the
 * offsets and the event records.  Null, misaligned, out-of-domain and too-small arguments are refused with a message that begins
 * "cluster_vertices:" before any launch. */
#define URSN_CLVTX_VI 17    /* int64 columns of a vertex record */
#define URSN_CLVTX_VR 5     /* fp64 columns of a vertex record */
#define URSN_CLVTX_IN 5     /* int64 columns of an incidence record */
#define URSN_CLVTX_EV 4     /* int64 columns of an event record */
#define URSN_CLVTX_INC_OVERFLOW 256 /* bit of *status */

typedef struct ursn_cluster_vtx_desc {  /* every pointer is a DEVICE pointer */
  int32_t ndim;                         /* 2 | 3 */
  int32_t spatial[3];                   /* extents in [1, 32768], prod < 2^31 (spatial[2] unused in 2-D) */
  int32_t n;                            /* events, 1..65535 */
  int32_t radius;                       /* 1..3 */
  int64_t m_total;                      /* list entries, < 2^30 */
  int64_t inc_cap;                      /* distinct incidences the scratch has room for, [0, 2^30) */
  const int64_t* offsets;               /* [n+1] */
  const int32_t* index;                 /* [m_total] strictly increasing per event */
  const int32_t* cluster;               /* [m_total] as ursn_cluster_voxels wrote it */
  const int64_t* table_offsets;         /* [n+1] as ursn_cluster_voxels wrote it */
  const int64_t* itab;                  /* [feat_cap][URSN_CLFEAT_I] as ursn_cluster_features wrote it for these lists */
  const double* rtab;                   /* [feat_cap][URSN_CLFEAT_R] */
  int64_t feat_cap;                     /* the cap of those tables */
  const uint8_t* cls;                   /* [K_total] the cluster table's cls, or null: every class mask is 0 */
  int32_t min_size;                     /* >= 1 */
  uint32_t class_mask;                  /* 0: rows of every class are eligible; else bit cls[r] decides, and cls must be given */
} ursn_cluster_vtx_desc;

typedef struct ursn_cluster_vtx_out {   /* DEVICE pointers */
  int64_t* vertex_offsets;              /* [n+1] */
  int64_t* vtx_itab;                    /* [cap_vertices][URSN_CLVTX_VI] */
  double* vtx_rtab;                     /* [cap_vertices][URSN_CLVTX_VR] */
  int64_t cap_vertices;
  int64_t* inc_offsets;                 /* [cap_vertices + 1] */
  int64_t* incidence;                   /* [inc_out_cap][URSN_CLVTX_IN] */
  int64_t inc_out_cap;
  int32_t* row_vertex;                  /* [cap_rows][2] */
  int64_t cap_rows;
  int64_t* event;                       /* [n][URSN_CLVTX_EV] */
  int32_t* status;                      /* [1] */
} ursn_cluster_vtx_out;

/* Bytes of scratch: 8-byte aligned, at least 8; 0 for n outside [1, 65535] or m_total / inc_cap outside [0, 2^30).  Host logic only. */
size_t ursn_cluster_vertices_scratch_bytes(int32_t n, int64_t m_total, int64_t inc_cap);
int ursn_cluster_vertices(const ursn_cluster_vtx_desc* d, const ursn_cluster_vtx_out* out, void* scratch, size_t scratch_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* URESNET_HIP_H */
