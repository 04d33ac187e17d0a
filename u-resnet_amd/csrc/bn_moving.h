// BatchNorm moving statistics (bn_moving.hip) as the two net plans see them: the part of slim.batch_norm the reference leaves
// dead (is_training is never False, UPDATE_OPS never run).
#pragma once
#include <vector>

#include "ursn_common.h"

// One BatchNorm layer of a plan: where its per-channel statistics live (separate arena pieces, padded to `stride` lanes) and
// where its [moving_mean[C] | moving_variance[C]] block starts inside the caller's flat moving buffer.
struct BnmEntry {
  float* mean;
  float* rstd;
  int32_t C, stride;
  int64_t off;
};

struct BnmState {
  std::vector<BnmEntry> host;     // ursn_query_layer order
  BnmEntry* table = nullptr;      // the same on the device (workspace), uploaded once at create
  // frozen mode: the conv kernels' own statistics finalise writes here instead of Layer::mean / rstd, one pair per stream
  // ([0] the caller's stream, [1] the side stream of the shortcut convs), never read
  float* scratch[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  int max_stride = 0;
  int64_t total = 0;              // 2 * sum C: floats of the moving buffer
  float* moving = nullptr;        // caller-owned, attached
  bool frozen = false;
  bool frozen_train = false;      // frozen only: the training entries run, with the fixed-statistics derivative (ursn_bn_frozen_train)
  int last_fwd = 0;               // 0: no forward has run, 1: batch statistics, 2: frozen
  float eps = 1e-3f;
};

// end of plan(): sizes the table / scratch pieces from st.host (entries filled by the plan; A.base == nullptr only counts)
void bnm_plan(BnmState& st, Arena& A);
// create: copies st.host to the device table (synchronous, like the plan's memsets)
int bnm_upload(BnmState& st);
// statistics pointers a forward conv hands to its finalise: the layer's own, or the scratch pair of `slot` while frozen
static inline float* bnm_mean(const BnmState& st, float* own, int slot) { return st.frozen ? st.scratch[slot][0] : own; }
static inline float* bnm_rstd(const BnmState& st, float* own, int slot) { return st.frozen ? st.scratch[slot][1] : own; }
// ONE launch each, all layers (grid.y = layer)
int bnm_launch_load(const BnmState& st, hipStream_t s);
int bnm_launch_update(const BnmState& st, double momentum, hipStream_t s);
