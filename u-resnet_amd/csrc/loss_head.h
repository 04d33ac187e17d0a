// Device loss head (loss_head.hip) as seen by the two net plans (net.hip, net_bf16.hip).
#pragma once
#include "ursn_common.h"

// One validated call of ursn_loss_head, cut into its launches so that a plan can record each of them when profiling.
struct LossHeadCall {
  ursn_vscores_desc d;
  const float *label, *weight;
  ursn_loss_desc spec;
  void* out; int ocs, odt;
  double* bs; int bs_blocks;
  float* out8;
  void* scratch;
  int nstages;   // filled by loss_head_prepare: 2 (main, finalise) without a Dice term, 3 (sums, finalise, gradient) with one
};
// Validates like the C entry point (nothing is launched on a refusal) and fills nstages.
int loss_head_prepare(LossHeadCall& c, size_t scratch_bytes);
// Stage i of a prepared call; *name: "losshead" (main / gradient pass), "losssums", "lossfinal"; *bytes: what the launch moves.
int loss_head_stage(const LossHeadCall& c, int i, hipStream_t s, const char** name, double* bytes);
size_t loss_head_scratch_bytes(int n, int64_t voxels);
// The spec's ranges alone (gamma 0 or >= 1, 0 <= smoothing < 1, dice_weight >= 0, dice_eps > 0): what a net-level call checks before its forward.
int loss_spec_check(const ursn_loss_desc* spec);

