// Host-side check of ursn_cluster_graph's argument checks and scratch query: a stand-alone program that links cluster_graph.hip
// alone (the two library hooks it needs are defined here) and makes only calls that are refused before any launch, with fake
// device pointers, so it needs no GPU.  Meant to be built with the sanitizers on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/cluster_graph.hip tools/micro/cluster_graph_check.cpp -o cluster_graph_check && ./cluster_graph_check
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/uresnet_hip.h"

static char g_err[512];
void ursn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
static long launches = 0;
void ursn_note_kernel(const char*) { ++launches; }

static long failures = 0, refused = 0;
static void* fake(uintptr_t a) { return (void*)(0x10000 + a); }

struct Case {
  ursn_cluster_graph_desc d;
  ursn_cluster_graph_out o;
  void* scratch;
  size_t bytes;
};

static Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.d.ndim = 3, c.d.spatial[0] = 7, c.d.spatial[1] = 9, c.d.spatial[2] = 11, c.d.n = 2, c.d.gap = 1, c.d.m_total = 10, c.d.edge_cap = 16;
  c.d.offsets = (const int64_t*)fake(0), c.d.index = (const int32_t*)fake(0x1000), c.d.cluster = (const int32_t*)fake(0x2000);
  c.d.table_offsets = (const int64_t*)fake(0x3000), c.d.value = (const float*)fake(0x4000), c.d.cls = (const uint8_t*)fake(0x5001);
  c.o.rows = (int64_t*)fake(0x10000), c.o.cap_rows = 10, c.o.groups = (int64_t*)fake(0x11000), c.o.cap_groups = 10;
  c.o.group_offsets = (int64_t*)fake(0x12000), c.o.event = (int64_t*)fake(0x13000), c.o.group = (int32_t*)fake(0x14000);
  c.o.edge_offsets = (int64_t*)fake(0x15000), c.o.edges = (int64_t*)fake(0x16000), c.o.edge_out_cap = 16;
  c.o.status = (int32_t*)fake(0x17000);
  c.scratch = fake(0x40000), c.bytes = 0;   // 0 bytes: whatever passes every other check is refused by the last one
  return c;
}

static void expect(const Case& c, const char* text) {
  g_err[0] = 0;
  const int rc = ursn_cluster_graph(&c.d, &c.o, c.scratch, c.bytes, nullptr);
  if (rc == 0 || strncmp(g_err, "cluster_graph:", 14) != 0 || !strstr(g_err, text)) {
    printf("FAILED: expected \"%s\", got rc %d \"%s\"\n", text, rc, g_err);
    ++failures;
  } else {
    ++refused;
  }
}

int main() {
  Case c = good();
  expect(c, "scratch of 0 bytes is too small");
  { g_err[0] = 0; if (ursn_cluster_graph(nullptr, &c.o, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  { g_err[0] = 0; if (ursn_cluster_graph(&c.d, nullptr, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  for (int n : {0, -1, 65536, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.n = n; expect(k, "outside [1, 65535]"); }
  for (int64_t m : {(int64_t)-1, (int64_t)1 << 31, INT64_MAX, INT64_MIN}) { Case k = good(); k.d.m_total = m; expect(k, "outside [0, 2^31)"); }
  for (int nd : {0, 1, 4, -3, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.ndim = nd; expect(k, "expected 2 or 3"); }
  for (int s : {0, -1, 32769, INT32_MAX, INT32_MIN}) {
    for (int ax = 0; ax < 3; ++ax) { Case k = good(); k.d.spatial[ax] = s; expect(k, "outside [1, 32768]"); }
  }
  { Case k = good(); k.d.spatial[0] = k.d.spatial[1] = k.d.spatial[2] = 32768; expect(k, "expected fewer than 2^31"); }
  { Case k = good(); k.d.spatial[0] = 2048, k.d.spatial[1] = 1024, k.d.spatial[2] = 1024; expect(k, "expected fewer than 2^31"); }
  for (int g : {0, 4, -1, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.gap = g; expect(k, "outside [1, 3]"); }
  for (int64_t e : {(int64_t)-1, (int64_t)1 << 30, INT64_MAX, INT64_MIN}) { Case k = good(); k.d.edge_cap = e; expect(k, "outside [0, 2^30)"); }
  for (int64_t cap : {(int64_t)-1, INT64_MIN}) {
    { Case k = good(); k.o.cap_rows = cap; expect(k, "cap_rows = "); }
    { Case k = good(); k.o.cap_groups = cap; expect(k, "cap_groups = "); }
    { Case k = good(); k.o.edge_out_cap = cap; expect(k, "edge_out_cap = "); }
  }
  { Case k = good(); k.d.offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.table_offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.index = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.d.cluster = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.o.status = nullptr; expect(k, "null out->status"); }
  { Case k = good(); k.o.group_offsets = nullptr; expect(k, "null out->group_offsets / out->event"); }
  { Case k = good(); k.o.event = nullptr; expect(k, "null out->group_offsets / out->event"); }
  { Case k = good(); k.o.group = nullptr; expect(k, "null out->group"); }
  { Case k = good(); k.o.rows = nullptr; expect(k, "null out->rows"); }
  { Case k = good(); k.o.groups = nullptr; expect(k, "null out->groups"); }
  { Case k = good(); k.o.edge_offsets = nullptr; expect(k, "out->edges needs out->edge_offsets"); }
  { Case k = good(); k.o.edges = nullptr; expect(k, "with null out->edges"); }
  { Case k = good(); k.scratch = nullptr; expect(k, "null scratch"); }
  // legal: no values or classes; 2-D at the largest extents and gap; counts only; no edge list; no rows or groups wanted; no
  // entries; the largest caps; no room for an edge
  { Case k = good(); k.d.value = nullptr; k.d.cls = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.ndim = 2; k.d.spatial[0] = k.d.spatial[1] = 32768; k.d.spatial[2] = INT32_MIN; k.d.gap = 3; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.edges = nullptr; k.o.edge_out_cap = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.edges = nullptr; k.o.edge_offsets = nullptr; k.o.edge_out_cap = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.edges = nullptr; k.o.edge_offsets = nullptr; k.o.edge_out_cap = INT64_MAX; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = k.o.cap_groups = 0; k.o.rows = k.o.groups = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.m_total = 0; k.d.index = k.d.cluster = nullptr; k.o.group = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = k.o.cap_groups = k.o.edge_out_cap = INT64_MAX; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.edge_cap = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.edge_cap = ((int64_t)1 << 30) - 1; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.offsets = (const int64_t*)fake(4); expect(k, "8-byte"); }
  { Case k = good(); k.d.table_offsets = (const int64_t*)fake(0x3004); expect(k, "8-byte"); }
  { Case k = good(); k.o.rows = (int64_t*)fake(0x10004); expect(k, "8-byte"); }
  { Case k = good(); k.o.groups = (int64_t*)fake(0x11004); expect(k, "8-byte"); }
  { Case k = good(); k.o.group_offsets = (int64_t*)fake(0x12004); expect(k, "8-byte"); }
  { Case k = good(); k.o.event = (int64_t*)fake(0x13004); expect(k, "8-byte"); }
  { Case k = good(); k.o.edge_offsets = (int64_t*)fake(0x15004); expect(k, "8-byte"); }
  { Case k = good(); k.o.edges = (int64_t*)fake(0x16004); expect(k, "8-byte"); }
  { Case k = good(); k.scratch = fake(0x40004); expect(k, "8-byte"); }
  { Case k = good(); k.d.index = (const int32_t*)fake(0x1002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.cluster = (const int32_t*)fake(0x2001); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.value = (const float*)fake(0x4002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.group = (int32_t*)fake(0x14002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.status = (int32_t*)fake(0x17001); expect(k, "4-byte aligned"); }
  // the query: 0 outside the domain; inside it at least 8, 8-byte granular, monotone in the list length and in edge_cap; 8 short
  // is refused
  const int64_t ms[] = {0, 1, 2, 3, 255, 256, 2047, 2048, 2049, 1000000, ((int64_t)1 << 31) - 1};
  const int64_t es[] = {0, 1, 2, 3, 1023, 1024, 1025, 1000000, ((int64_t)1 << 30) - 1};
  for (int n : {1, 2, 65535}) {
    size_t prev_e = 0;
    for (int64_t e : es) {
      size_t prev = 0;
      for (int64_t m : ms) {
        const size_t b = ursn_cluster_graph_scratch_bytes(n, m, m, m, e);
        if (b < 8 || b % 8 != 0 || b < prev || b < (size_t)m * 8 || b < (size_t)e * 8) {
          printf("FAILED: query(%d, %lld, %lld) = %zu\n", n, (long long)m, (long long)e, b);
          ++failures;
        }
        prev = b;
        Case k = good();
        k.d.n = n, k.d.m_total = m, k.d.edge_cap = e, k.o.cap_rows = k.o.cap_groups = m, k.o.edge_out_cap = e, k.bytes = b - 8;
        expect(k, "is too small");
      }
      const size_t at = ursn_cluster_graph_scratch_bytes(n, 1000, 1000, 1000, e);
      if (at < prev_e) { printf("FAILED: the query falls with edge_cap at %lld\n", (long long)e); ++failures; }
      prev_e = at;
    }
  }
  if (ursn_cluster_graph_scratch_bytes(0, 1, 1, 1, 1) || ursn_cluster_graph_scratch_bytes(65536, 1, 1, 1, 1) ||
      ursn_cluster_graph_scratch_bytes(1, -1, 1, 1, 1) || ursn_cluster_graph_scratch_bytes(1, (int64_t)1 << 31, 1, 1, 1) ||
      ursn_cluster_graph_scratch_bytes(1, 1, -1, 1, 1) || ursn_cluster_graph_scratch_bytes(1, 1, 1, -1, 1) ||
      ursn_cluster_graph_scratch_bytes(1, 1, 1, 1, -1) || ursn_cluster_graph_scratch_bytes(1, 1, 1, 1, (int64_t)1 << 30) ||
      ursn_cluster_graph_scratch_bytes(1, INT64_MAX, INT64_MAX, 1, INT64_MAX) ||
      ursn_cluster_graph_scratch_bytes(INT32_MIN, INT64_MIN, INT64_MIN, INT64_MIN, INT64_MIN)) {
    printf("FAILED: the query answers outside its domain\n");
    ++failures;
  }
  if (launches) { printf("FAILED: %ld launches noted\n", launches); ++failures; }
  printf("%ld refused, %ld launches\n", refused, launches);
  printf(failures ? "FAILED: %ld\n" : "argument checks consistent\n", failures);
  return failures != 0;
}
