// The U-ResNet of lib/uresnet.py:22-123 + lib/resnet_module.py:10-87 as ONE table: everything about the network that follows
// from the configuration alone (no precision, no arena, no URSN_* switch).  Both plans (net.hip, net_bf16.hip) walk it and add
// only what is their own; the host queries (ursn_query_layer / _concat / ursn_param / ...) answer from it without a plan.
// Host code only (topology.hip has no device code and no HIP call; tools/micro/topology_check.cpp links it alone).
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "ursn_common.h"

struct TopoLayer {   // one conv-like layer (+ its BatchNorm): a row of ursn_query_layer, in parameter order
  std::string name;  // with the UResNet/ prefix
  int kind = 0;      // 0 conv, 1 transposed conv
  int k = 3, stride = 1, cin = 0, cout = 0, lin = 0, lout = 0;   // real channel counts (parameter tensor), levels in / out
  int relu = 0;      // activation_fn of the slim layer call (conv0 / deconv / conv1: ReLU; all others None)
  int64_t w_off = 0, b_off = 0, w_n = 0;   // weights [w_off, w_off + w_n) and beta [b_off, b_off + cout) in the flat parameters
};

enum TopoSource { TOPO_SRC_PREV = 0, TOPO_SRC_CONV0 = 1, TOPO_SRC_CONCAT = 2 };

struct TopoUnit {    // one resnet_module (lib/resnet_module.py), execution order
  std::string scope;               // with the UResNet/ prefix
  int sc = -1, c1 = -1, c2 = -1;   // layer indices: shortcut (-1: identity), resnet_conv1, resnet_conv2
  int lin = 0, lout = 0, co = 0, stride = 1;
  int src = TOPO_SRC_PREV;         // the input: the previous unit's output, conv0's, or the concat of decoder step src_step
  int src_step = -1;
  int skip_of = -1;                // >= 0: the output is the skip half of decoder step skip_of's concat (cat_names[].second)
};

// the part the plans keep as fields of their own (assigned whole from the table)
struct TopoShape {
  int ndim = 0, nlev = 0;
  int ldim[8][3] = {};   // spatial dims per level (3 entries, leading 1 for 2-D)
  int64_t lvox[8] = {};  // voxels per image per level
  std::vector<int> deconv;   // layer index per decoder step
  std::vector<std::pair<std::string, std::string>> cat_names;   // per decoder step: producers of [first | second] channel halves
  int conv0 = -1, conv1 = -1, conv2 = -1;
  int64_t n_params = 0;
};

struct Topology : TopoShape {
  std::vector<TopoLayer> layers;
  std::vector<TopoUnit> units;   // encoder units then decoder units
};

// Fills `out`, or refuses the configuration (return code 2, ursn_last_error) with the checks of the plan act_dtype selects, in
// that plan's order; a refused `out` is empty and safe to destroy.
int topology_build(const ursn_config& cfg, Topology& out);
// ursn_param: tensor 2 * layer is the layer's weights, 2 * layer + 1 its BatchNorm beta
int topology_param(const Topology& T, int64_t index, ursn_param_info* out);

// The suffixes of ursn_tensor names, stripped off `name` in this order (each at most once); returns the kinds found.
enum TensorKind { TK_DZ = 1, TK_Z = 2, TK_GRAD2 = 4, TK_GRAD = 8, TK_MEAN = 16, TK_RSTD = 32 };
unsigned tensor_name_kinds(std::string& name, bool with_grad2);
