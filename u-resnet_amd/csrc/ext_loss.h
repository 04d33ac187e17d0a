// External loss boundary (ext_loss.hip) as seen by the two net plans (net.hip, net_bf16.hip).
#pragma once
#include "ursn_common.h"

// ursn_logits_dense on a stream: conv2's stored operands -> compact fp32 logits [n, voxels, ncls].  Validates like the C entry point.
int launch_logits_dense(const ursn_vscores_desc* d, float* logits_out, hipStream_t s);

// ursn_dlogits_pack on a stream, plus the net-level form: bs_partial != nullptr also writes the logits layer's BatchNorm-backward
// partials the plan's head would have written from the STORED values (fp32: [bs_blocks][3][4] doubles, needs out_cstride 4 and
// <= 4 classes; bf16: [bs_blocks][3][8]) -- same partition of the voxels over bs_blocks workgroups of 256 threads, same order of
// every sum.  z (the layer's raw output in the layout of `out`), mean and rstd are needed for the partials only.
int launch_dlogits_pack(const float* dlogits, int32_t n, int64_t voxels, int32_t ncls, void* out, int32_t out_cstride, int32_t dtype,
                        const void* z, const float* mean, const float* rstd, double* bs_partial, int bs_blocks, hipStream_t s);

// ursn_conv0_input_grad on a stream.
int launch_conv0_input_grad(int32_t ndim, const int32_t* spatial, int32_t n, int32_t cin, int32_t F, const void* dz, int32_t dz_cstride,
                            int32_t dtype, const float* w, float* dinput_out, hipStream_t s);
