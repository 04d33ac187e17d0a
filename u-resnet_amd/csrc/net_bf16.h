// bf16 mixed-precision plan (net_bf16.hip) as seen by the C-ABI dispatch in net.hip.
#pragma once
#include "ursn_common.h"

struct ursn_bnet;
int bnet_query(const ursn_config* cfg, ursn_sizes* out);
int bnet_create(const ursn_config* cfg, float* params, float* grads, void* workspace, size_t workspace_bytes, ursn_bnet** out);
void bnet_destroy(ursn_bnet* n);
const ursn_sizes* bnet_sizes(const ursn_bnet* n);
float* bnet_metrics(ursn_bnet* n);
struct BnmState;
BnmState* bnet_bnm(ursn_bnet* n);   // BatchNorm moving statistics of the plan (bn_moving.h)
int bnet_bn_update(ursn_bnet* n, double momentum, hipStream_t s);   // ursn_bn_update's launch, recorded when profiling
// mode 0: forward + loss + backward (gradients accumulate); 1: forward + loss; 2: forward + softmax / ana labels
int bnet_step(ursn_bnet* n, const float* data, const float* label, const float* weight, int N, int mode, float* softmax_out,
              float* labels_out, hipStream_t s);
// ursn_infer_voxels: forward, the dense head for the accuracies only when label != nullptr, the gather head (voxel_io.hip) on
// conv2's operands; enqueues only
int bnet_infer_voxels(ursn_bnet* n, const float* data, const float* label, int N, const int64_t* offsets, const int32_t* index,
                      int64_t m_total, float* scores_out, uint8_t* pred_out, uint8_t* ana_out, hipStream_t s);
// ursn_infer_stats: forward, the dense head only with dense_head, the class statistics (ana_stats.hip) on conv2's z / mean / rstd
int bnet_infer_stats(ursn_bnet* n, const float* data, const float* label, int N, bool dense_head, float* labels_out,
                     float* softmax_out, const ursn_class_stats_out* stats, hipStream_t s);
// external loss boundary (ext_loss.hip): forward + logits_dense without the head; dlogits_pack + backward (+ conv0_input_grad)
int bnet_forward_logits(ursn_bnet* n, const float* data, int N, float* logits_out, hipStream_t s);
int bnet_backward_logits(ursn_bnet* n, const float* data, const float* dlogits, int N, float* dinput_out, hipStream_t s);
// ursn_accum_step_loss (mode 0) / ursn_eval_loss (mode 1): bnet_step with the loss head (loss_head.hip) in the place of the head
// *ran_forward: set once the call's arguments were accepted and the forward's launches begin
int bnet_step_loss(ursn_bnet* n, const float* data, const float* label, const float* weight, int N, const ursn_loss_desc* spec,
                   int mode, hipStream_t s, bool* ran_forward);
int bnet_tensor(const ursn_bnet* n, const char* name, void** ptr, int64_t* voxels, int32_t* channels, int32_t* cstride);
// the plan's per-launch HIP-event log (prof_log.h; ursn_profile_enable / ursn_profile_read) and the weight-gradient stream switch
struct ProfLog;
ProfLog* bnet_prof(ursn_bnet* n);
int bnet_set_wgrad_overlap(ursn_bnet* n, int on);
