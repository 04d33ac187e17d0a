// Host-side memory and consistency check of the topology table: a stand-alone program that links topology.hip alone (the one
// library hook it needs is defined here), builds the table for the configuration matrix of tools/plan_snapshot.py -- refused
// configurations included -- and checks what every reader of the table relies on.  Meant to be built with the sanitizers on
// the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/topology.hip tools/micro/topology_check.cpp -o topology_check && ./topology_check
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <set>

#include "../../u-resnet_amd/csrc/topology.h"

static char g_err[512];
void ursn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static long failures = 0, accepted = 0, refused = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (++failures <= 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                                 \
  } while (0)

static void check(const ursn_config& c) {
  char what[128];
  snprintf(what, sizeof(what), "ndim %d sp %d,%d,%d cin %d F %d ncls %d ns %d mb %d dtype %d", c.ndim, c.spatial[0], c.spatial[1],
           c.spatial[2], c.cin, c.base_filters, c.num_class, c.num_strides, c.max_batch, c.act_dtype);
  g_err[0] = 0;
  Topology T;
  const int rc = topology_build(c, T);
  if (rc != 0) {
    ++refused;
    CHECK(g_err[0] != 0, "%s: refused without a message", what);
    return;   // T is destroyed here
  }
  ++accepted;
  const int nl = (int)T.layers.size();
  CHECK(T.nlev == c.num_strides + 1 && T.ndim == c.ndim, "%s", what);
  int64_t at = 0;   // the parameter ranges tile [0, n_params) in layer order
  std::set<std::string> names;
  for (const TopoLayer& L : T.layers) {
    CHECK(L.w_off == at && L.w_n > 0 && L.b_off == at + L.w_n, "%s: %s at %lld", what, L.name.c_str(), (long long)at);
    at = L.b_off + L.cout;
    CHECK(names.insert(L.name).second, "%s: duplicate %s", what, L.name.c_str());
    CHECK(L.lin >= 0 && L.lin < T.nlev && L.lout >= 0 && L.lout < T.nlev, "%s: %s levels", what, L.name.c_str());
  }
  CHECK(at == T.n_params, "%s: %lld != n_params %lld", what, (long long)at, (long long)T.n_params);
  auto layer_ok = [&](int li) { return li >= 0 && li < nl; };
  CHECK(layer_ok(T.conv0) && layer_ok(T.conv1) && layer_ok(T.conv2), "%s: conv0/1/2", what);
  CHECK((int)T.deconv.size() == c.num_strides && T.cat_names.size() == T.deconv.size(), "%s: decoder steps", what);
  for (const TopoUnit& u : T.units) {
    CHECK((u.sc == -1 || layer_ok(u.sc)) && layer_ok(u.c1) && layer_ok(u.c2), "%s: %s layers", what, u.scope.c_str());
    CHECK(u.lin >= 0 && u.lin < T.nlev && u.lout >= 0 && u.lout < T.nlev, "%s: %s levels", what, u.scope.c_str());
    CHECK(u.src != TOPO_SRC_CONCAT || (u.src_step >= 0 && u.src_step < (int)T.deconv.size()), "%s: %s source", what, u.scope.c_str());
    CHECK(u.skip_of < (int)T.deconv.size(), "%s: %s skip", what, u.scope.c_str());
    if (u.skip_of >= 0) CHECK(T.cat_names[u.skip_of].second == u.scope, "%s: %s skip name", what, u.scope.c_str());
  }
  for (size_t i = 0; i < T.deconv.size(); ++i) {
    CHECK(layer_ok(T.deconv[i]), "%s: deconv %zu", what, i);
    if (layer_ok(T.deconv[i])) CHECK(T.cat_names[i].first == T.layers[T.deconv[i]].name, "%s: concat %zu", what, i);
    bool produced = layer_ok(T.conv0) && T.cat_names[i].second == T.layers[T.conv0].name;   // the skip: conv0 or a unit
    for (const TopoUnit& u : T.units) produced = produced || (u.skip_of == (int)i && u.scope == T.cat_names[i].second);
    CHECK(produced, "%s: concat %zu has no second producer", what, i);
  }
  ursn_param_info info;
  CHECK(topology_param(T, 2 * (int64_t)nl, &info) != 0 && topology_param(T, -1, &info) != 0, "%s: param range", what);
  CHECK(topology_param(T, 2 * (int64_t)nl - 1, &info) == 0 && info.offset + info.nelem == T.n_params, "%s: last param", what);
}

int main() {
  const int cins[] = {1, 2, 3, 4, 8}, widths[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32}, classes[] = {1, 2, 3, 4, 6, 7, 8, 9};
  const int strides[] = {1, 3, 5}, batches[] = {1, 2, 4};
  ursn_config c;
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int ndim = 2; ndim <= 3; ++ndim)
      for (int cin : cins) for (int F : widths) for (int ncls : classes) for (int ns : strides) for (int mb : batches) {
        memset(&c, 0, sizeof(c));
        c.ndim = ndim;
        for (int j = 0; j < 3; ++j) c.spatial[j] = j < ndim ? 32 : 1;
        c.cin = cin; c.base_filters = F; c.num_class = ncls; c.num_strides = ns; c.max_batch = mb; c.trainable = 1;
        c.act_dtype = dtype;
        check(c);
      }
  // the workload shapes of bench.py
  const int bench[][6] = {{3, 192, 8, 3, 4, 0}, {2, 512, 16, 5, 16, 0}, {2, 256, 16, 3, 4, 0}, {3, 64, 8, 3, 2, 0},
                          {3, 256, 8, 3, 4, 1}, {3, 256, 8, 3, 4, 0}, {3, 64, 8, 3, 2, 1}};
  for (const auto& b : bench) {
    memset(&c, 0, sizeof(c));
    c.ndim = b[0];
    for (int j = 0; j < 3; ++j) c.spatial[j] = j < b[0] ? b[1] : 1;
    c.cin = 1; c.base_filters = b[2]; c.num_class = b[3]; c.num_strides = 5; c.max_batch = b[4]; c.act_dtype = b[5];
    check(c);
  }
  // every refusal of its own: dims, strides, channels, width, classes, batch, spatial size
  memset(&c, 0, sizeof(c));
  c.ndim = 3; c.spatial[0] = c.spatial[1] = c.spatial[2] = 32; c.cin = 1; c.base_filters = 8; c.num_class = 3; c.num_strides = 5;
  c.max_batch = 1;
  const long before = refused;
  { ursn_config d = c; d.ndim = 4; check(d); }
  { ursn_config d = c; d.ndim = 0; check(d); }
  { ursn_config d = c; d.num_strides = 0; check(d); }
  { ursn_config d = c; d.num_strides = 6; check(d); }
  { ursn_config d = c; d.cin = 0; check(d); }
  { ursn_config d = c; d.base_filters = 0; check(d); }
  { ursn_config d = c; d.num_class = 0; check(d); }
  { ursn_config d = c; d.max_batch = 0; check(d); }
  { ursn_config d = c; d.spatial[1] = 48; check(d); }
  { ursn_config d = c; d.spatial[2] = 0; check(d); }
  { ursn_config d = c; d.spatial[0] = -32; check(d); }
  if (refused - before != 11) { printf("FAILED: %ld of the 11 single refusals\n", refused - before); ++failures; }
  // the suffixes of tensor names
  std::string s = "UResNet/conv0:grad2";
  if (tensor_name_kinds(s, false) != 0 || s != "UResNet/conv0:grad2") { printf("FAILED: :grad2 without second gradients\n"); ++failures; }
  if (tensor_name_kinds(s, true) != TK_GRAD2 || s != "UResNet/conv0") { printf("FAILED: :grad2\n"); ++failures; }
  s = ":z";
  if (tensor_name_kinds(s, true) != 0 || s != ":z") { printf("FAILED: a bare suffix is a name\n"); ++failures; }
  s = "a:dz";
  if (tensor_name_kinds(s, true) != TK_DZ || s != "a") { printf("FAILED: :dz\n"); ++failures; }
  printf("%ld accepted, %ld refused\n", accepted, refused);
  printf(failures ? "FAILED: %ld\n" : "topology table consistent\n", failures);
  return failures != 0;
}
