// The network's shape as one table (topology.h).  Host code only.
#include <stdio.h>
#include <string.h>

#include "topology.h"

int topology_build(const ursn_config& c, Topology& T) {
  T = Topology();
  URSN_REQUIRE(c.ndim == 2 || c.ndim == 3, "len(dims) must be 3 (H,W,C) or 4 (H,W,D,C)");
  // the decoder scopes are the reference's literal 'resnet_module%d' % (step + 5) (lib/uresnet.py:100): with more than 5
  // strides they collide with the encoder's names (TensorFlow raises on the duplicate variable scope as well)
  URSN_REQUIRE(c.num_strides >= 1 && c.num_strides <= 5, "num_strides %d out of range [1,5]", c.num_strides);
  if (c.act_dtype == 1) {   // the bf16 plan's own domain (net_bf16.hip): checked here to keep the order of the refusals
    URSN_REQUIRE(c.cin == 1, "bf16 path: one input channel (the reference's data), got %d", c.cin);
    URSN_REQUIRE(c.base_filters >= 8 && c.base_filters % 8 == 0, "bf16 path: base_num_outputs must be a multiple of 8, got %d", c.base_filters);
  } else {
    URSN_REQUIRE(c.cin >= 1, "input channels (dims[-1]) must be >= 1, got %d", c.cin);
    URSN_REQUIRE(c.base_filters >= 1, "base_num_outputs must be >= 1, got %d", c.base_filters);
  }
  URSN_REQUIRE(c.num_class >= 1 && c.num_class <= 8, "num_class %d out of range [1,8] (the head's 8-channel logits piece)", c.num_class);
  URSN_REQUIRE(c.max_batch >= 1, "max_batch must be >= 1, got %d", c.max_batch);
  const int ns = c.num_strides, F = c.base_filters, lead = 3 - c.ndim;
  for (int j = 0; j < c.ndim; ++j)
    URSN_REQUIRE(c.spatial[j] > 0 && c.spatial[j] % (1 << ns) == 0,
                 "spatial size %d not divisible by 2^%d (deconv/skip shapes would differ)", c.spatial[j], ns);
  for (int l = 0; l <= ns; ++l) {
    T.lvox[l] = 1;
    for (int j = 0; j < 3; ++j) {
      T.ldim[l][j] = j < lead ? 1 : c.spatial[j - lead] >> l;
      T.lvox[l] *= T.ldim[l][j];
    }
  }
  T.ndim = c.ndim;
  T.nlev = ns + 1;

  auto add_layer = [&](const std::string& name, int kind, int k, int s, int ci, int co, int lin, int lout, int relu) {
    TopoLayer L;
    L.name = "UResNet/" + name;
    L.kind = kind; L.k = k; L.stride = s; L.cin = ci; L.cout = co; L.lin = lin; L.lout = lout; L.relu = relu;
    int64_t taps = 1;
    for (int j = 0; j < c.ndim; ++j) taps *= k;
    L.w_n = taps * ci * co;
    L.w_off = T.n_params; T.n_params += L.w_n;
    L.b_off = T.n_params; T.n_params += co;
    T.layers.push_back(L);
    return (int)T.layers.size() - 1;
  };
  auto add_unit = [&](const std::string& scope, int ci, int co, int s, int lin, int lout, int src, int src_step) -> TopoUnit& {
    TopoUnit u;
    u.scope = "UResNet/" + scope;
    u.lin = lin; u.lout = lout; u.co = co; u.stride = s; u.src = src; u.src_step = src_step;
    if (!(ci == co && s == 1)) u.sc = add_layer(scope + "/shortcut", 0, 1, s, ci, co, lin, lout, 0);
    u.c1 = add_layer(scope + "/resnet_conv1", 0, 3, s, ci, co, lin, lout, 0);
    u.c2 = add_layer(scope + "/resnet_conv2", 0, 3, 1, co, co, lout, lout, 0);
    T.units.push_back(u);
    return T.units.back();
  };

  T.conv0 = add_layer("conv0", 0, 3, 1, c.cin, F, 0, 0, 1);
  std::vector<std::string> skip_name(ns + 1);   // producer of the encoder feature map at each level
  skip_name[0] = "UResNet/conv0";
  char sc[64];
  int C = F;
  for (int step = 0; step < ns; ++step) {
    snprintf(sc, sizeof(sc), "resnet_module%d/module1", step);
    add_unit(sc, C, 2 * C, 2, step, step + 1, step ? TOPO_SRC_PREV : TOPO_SRC_CONV0, -1);
    C *= 2;
    snprintf(sc, sizeof(sc), "resnet_module%d/module2", step);
    TopoUnit& u = add_unit(sc, C, C, 1, step + 1, step + 1, TOPO_SRC_PREV, -1);
    if (step + 1 < ns) u.skip_of = ns - 2 - step;
    skip_name[step + 1] = u.scope;
  }
  for (int i = 0; i < ns; ++i) {   // decoder step i lives at level ns-1-i
    const int lvl = ns - 1 - i, co = C / 2;
    snprintf(sc, sizeof(sc), "deconv%d", i);
    T.deconv.push_back(add_layer(sc, 1, 3, 2, C, co, lvl + 1, lvl, 1));
    T.cat_names.push_back({T.layers[T.deconv[i]].name, skip_name[lvl]});   // tf.concat([deconv_i, skip]) (lib/uresnet.py:81)
    snprintf(sc, sizeof(sc), "resnet_module%d/module1", i + 5);
    add_unit(sc, 2 * co, co, 1, lvl, lvl, TOPO_SRC_CONCAT, i);
    snprintf(sc, sizeof(sc), "resnet_module%d/module2", i + 5);
    add_unit(sc, co, co, 1, lvl, lvl, TOPO_SRC_PREV, -1);
    C = co;
  }
  T.conv1 = add_layer("conv1", 0, 3, 1, C, F, 0, 0, 1);
  T.conv2 = add_layer("conv2", 0, 3, 1, F, c.num_class, 0, 0, 0);
  return 0;
}

int topology_param(const Topology& T, int64_t index, ursn_param_info* out) {
  URSN_REQUIRE(index >= 0 && index < 2 * (int64_t)T.layers.size(), "param: index %lld out of range", (long long)index);
  const TopoLayer& L = T.layers[index / 2];
  memset(out, 0, sizeof(*out));
  if (index % 2 == 0) {
    snprintf(out->name, sizeof(out->name), "%s/weights", L.name.c_str());
    out->offset = L.w_off; out->nelem = L.w_n; out->rank = T.ndim + 2;
    for (int j = 0; j < T.ndim; ++j) out->shape[j] = L.k;
    out->shape[T.ndim] = L.kind ? L.cout : L.cin;
    out->shape[T.ndim + 1] = L.kind ? L.cin : L.cout;
  } else {
    snprintf(out->name, sizeof(out->name), "%s/BatchNorm/beta", L.name.c_str());
    out->offset = L.b_off; out->nelem = L.cout; out->rank = 1; out->shape[0] = L.cout;
  }
  return 0;
}

unsigned tensor_name_kinds(std::string& name, bool with_grad2) {
  static const struct { const char* suffix; unsigned kind; } table[] = {
      {":dz", TK_DZ}, {":z", TK_Z}, {":grad2", TK_GRAD2}, {":grad", TK_GRAD}, {":mean", TK_MEAN}, {":rstd", TK_RSTD}};
  unsigned kinds = 0;
  for (const auto& e : table) {
    const size_t n = strlen(e.suffix);
    if (e.kind == TK_GRAD2 && !with_grad2) continue;
    if (name.size() > n && name.compare(name.size() - n, n, e.suffix) == 0) { kinds |= e.kind; name.resize(name.size() - n); }
  }
  return kinds;
}
