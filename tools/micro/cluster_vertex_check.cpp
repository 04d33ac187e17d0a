// Host-side check of ursn_cluster_vertices' argument checks and scratch query: a stand-alone program that links cluster_vertex.hip
// alone (the two library hooks it needs are defined here) and makes only calls that are refused before any launch, with fake
// device pointers, so it needs no GPU.  Meant to be built with the sanitizers on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/cluster_vertex.hip tools/micro/cluster_vertex_check.cpp -o cluster_vertex_check && ./cluster_vertex_check
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
  ursn_cluster_vtx_desc d;
  ursn_cluster_vtx_out o;
  void* scratch;
  size_t bytes;
};

static Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.d.ndim = 3, c.d.spatial[0] = 7, c.d.spatial[1] = 9, c.d.spatial[2] = 11, c.d.n = 2, c.d.radius = 2, c.d.m_total = 10, c.d.inc_cap = 64;
  c.d.offsets = (const int64_t*)fake(0), c.d.index = (const int32_t*)fake(0x1000), c.d.cluster = (const int32_t*)fake(0x2000);
  c.d.table_offsets = (const int64_t*)fake(0x3000), c.d.itab = (const int64_t*)fake(0x5000), c.d.rtab = (const double*)fake(0x6000);
  c.d.feat_cap = 10, c.d.cls = (const uint8_t*)fake(0x7000), c.d.min_size = 3, c.d.class_mask = 6;
  c.o.vertex_offsets = (int64_t*)fake(0x10000), c.o.vtx_itab = (int64_t*)fake(0x11000), c.o.vtx_rtab = (double*)fake(0x12000);
  c.o.cap_vertices = 20, c.o.inc_offsets = (int64_t*)fake(0x13000), c.o.incidence = (int64_t*)fake(0x14000), c.o.inc_out_cap = 64;
  c.o.row_vertex = (int32_t*)fake(0x15000), c.o.cap_rows = 10, c.o.event = (int64_t*)fake(0x16000), c.o.status = (int32_t*)fake(0x17000);
  c.scratch = fake(0x40000), c.bytes = 0;   // 0 bytes: whatever passes every other check is refused by the last one
  return c;
}

static void expect(const Case& c, const char* text) {
  g_err[0] = 0;
  const int rc = ursn_cluster_vertices(&c.d, &c.o, c.scratch, c.bytes, nullptr);
  if (rc == 0 || strncmp(g_err, "cluster_vertices:", 17) != 0 || !strstr(g_err, text)) {
    printf("FAILED: expected \"%s\", got rc %d \"%s\"\n", text, rc, g_err);
    ++failures;
  } else {
    ++refused;
  }
}

int main() {
  Case c = good();
  expect(c, "scratch of 0 bytes is too small");
  { g_err[0] = 0; if (ursn_cluster_vertices(nullptr, &c.o, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  { g_err[0] = 0; if (ursn_cluster_vertices(&c.d, nullptr, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  for (int n : {0, -1, 65536, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.n = n; expect(k, "outside [1, 65535]"); }
  for (int64_t m : {(int64_t)-1, (int64_t)1 << 30, (int64_t)1 << 31, INT64_MAX, INT64_MIN}) {
    Case k = good(); k.d.m_total = m; expect(k, "m_total = ");
  }
  for (int nd : {0, 1, 4, -3, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.ndim = nd; expect(k, "expected 2 or 3"); }
  for (int s : {0, -1, 32769, INT32_MAX, INT32_MIN}) {
    for (int ax = 0; ax < 3; ++ax) { Case k = good(); k.d.spatial[ax] = s; expect(k, "outside [1, 32768]"); }
  }
  { Case k = good(); k.d.spatial[0] = k.d.spatial[1] = k.d.spatial[2] = 32768; expect(k, "expected fewer than 2^31"); }
  { Case k = good(); k.d.spatial[0] = 2048, k.d.spatial[1] = 1024, k.d.spatial[2] = 1024; expect(k, "expected fewer than 2^31"); }
  for (int r : {0, 4, -1, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.radius = r; expect(k, "outside [1, 3]"); }
  for (int s : {0, -1, INT32_MIN}) { Case k = good(); k.d.min_size = s; expect(k, "min_size = "); }
  for (int64_t cap : {(int64_t)-1, (int64_t)1 << 30, INT64_MAX, INT64_MIN}) { Case k = good(); k.d.inc_cap = cap; expect(k, "inc_cap = "); }
  for (int64_t cap : {(int64_t)-1, INT64_MIN}) {
    { Case k = good(); k.d.feat_cap = cap; expect(k, "feat_cap = "); }
    { Case k = good(); k.o.cap_rows = cap; expect(k, "cap_rows = "); }
    { Case k = good(); k.o.cap_vertices = cap; expect(k, "cap_vertices = "); }
    { Case k = good(); k.o.inc_out_cap = cap; expect(k, "inc_out_cap = "); }
  }
  { Case k = good(); k.d.offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.table_offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.index = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.d.cluster = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.d.itab = nullptr; expect(k, "null itab / rtab"); }
  { Case k = good(); k.d.rtab = nullptr; expect(k, "null itab / rtab"); }
  for (uint32_t mask : {1u, 6u, 0x80000000u, 0xFFFFFFFFu}) { Case k = good(); k.d.cls = nullptr; k.d.class_mask = mask; expect(k, "needs cls"); }
  { Case k = good(); k.o.status = nullptr; expect(k, "null out->status"); }
  { Case k = good(); k.o.vertex_offsets = nullptr; expect(k, "null out->vertex_offsets / out->inc_offsets / out->event"); }
  { Case k = good(); k.o.inc_offsets = nullptr; expect(k, "null out->vertex_offsets / out->inc_offsets / out->event"); }
  { Case k = good(); k.o.event = nullptr; expect(k, "null out->vertex_offsets / out->inc_offsets / out->event"); }
  { Case k = good(); k.o.vtx_itab = nullptr; expect(k, "null out->vtx_itab / out->vtx_rtab"); }
  { Case k = good(); k.o.vtx_rtab = nullptr; expect(k, "null out->vtx_itab / out->vtx_rtab"); }
  { Case k = good(); k.o.incidence = nullptr; expect(k, "null out->incidence"); }
  { Case k = good(); k.o.row_vertex = nullptr; expect(k, "null out->row_vertex"); }
  { Case k = good(); k.scratch = nullptr; expect(k, "null scratch"); }
  // legal: no cls; cls at an odd address; 2-D at the largest extents; the ends of every range; no rows, vertices, incidences or
  // object records; no entries; the largest caps
  { Case k = good(); k.d.cls = nullptr; k.d.class_mask = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.cls = (const uint8_t*)fake(0x7003); k.d.class_mask = 0xFFFFFFFFu; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.ndim = 2; k.d.spatial[0] = k.d.spatial[1] = 32768; k.d.spatial[2] = INT32_MIN; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.radius = 1, k.d.min_size = 1; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.radius = 3, k.d.min_size = INT32_MAX; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = 0; k.o.row_vertex = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_vertices = 0; k.o.vtx_itab = nullptr; k.o.vtx_rtab = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.inc_out_cap = 0; k.o.incidence = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.inc_cap = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.feat_cap = 0; k.d.itab = nullptr; k.d.rtab = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.m_total = 0; k.d.index = k.d.cluster = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = k.o.cap_vertices = k.o.inc_out_cap = k.d.feat_cap = INT64_MAX; k.d.inc_cap = ((int64_t)1 << 30) - 1;
    k.d.m_total = ((int64_t)1 << 30) - 1; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.offsets = (const int64_t*)fake(4); expect(k, "8-byte"); }
  { Case k = good(); k.d.table_offsets = (const int64_t*)fake(0x3004); expect(k, "8-byte"); }
  { Case k = good(); k.d.itab = (const int64_t*)fake(0x5004); expect(k, "8-byte"); }
  { Case k = good(); k.d.rtab = (const double*)fake(0x6004); expect(k, "8-byte"); }
  { Case k = good(); k.o.vertex_offsets = (int64_t*)fake(0x10004); expect(k, "8-byte"); }
  { Case k = good(); k.o.vtx_itab = (int64_t*)fake(0x11004); expect(k, "8-byte"); }
  { Case k = good(); k.o.vtx_rtab = (double*)fake(0x12004); expect(k, "8-byte"); }
  { Case k = good(); k.o.inc_offsets = (int64_t*)fake(0x13004); expect(k, "8-byte"); }
  { Case k = good(); k.o.incidence = (int64_t*)fake(0x14004); expect(k, "8-byte"); }
  { Case k = good(); k.o.event = (int64_t*)fake(0x16004); expect(k, "8-byte"); }
  { Case k = good(); k.scratch = fake(0x40004); expect(k, "8-byte"); }
  { Case k = good(); k.d.index = (const int32_t*)fake(0x1002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.cluster = (const int32_t*)fake(0x2001); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.row_vertex = (int32_t*)fake(0x15002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.status = (int32_t*)fake(0x17001); expect(k, "4-byte aligned"); }
  // the query: 0 outside the domain; inside it at least 8, 8-byte granular, monotone in the list length and in the incidence cap,
  // room for the two key arrays (16 bytes per entry) and a slot per incidence (32 bytes); 8 short is refused
  const int64_t ms[] = {0, 1, 2, 3, 255, 256, 2047, 2048, 2049, 1000000, ((int64_t)1 << 30) - 1};
  for (int n : {1, 2, 65535}) {
    size_t below = 0;
    for (int64_t ic : {(int64_t)0, (int64_t)1000, ((int64_t)1 << 30) - 1}) {
      size_t prev = 0;
      for (int64_t m : ms) {
        const size_t b = ursn_cluster_vertices_scratch_bytes(n, m, ic);
        if (b < 8 || b % 8 != 0 || b < prev || b < (size_t)m * 16 + (size_t)ic * 32) {
          printf("FAILED: query(%d, %lld, %lld) = %zu\n", n, (long long)m, (long long)ic, b);
          ++failures;
        }
        prev = b;
        Case k = good();
        k.d.n = n, k.d.m_total = m, k.d.inc_cap = ic, k.bytes = b - 8;
        expect(k, "is too small");
      }
      if (prev < below) { printf("FAILED: the query is not monotone in inc_cap\n"); ++failures; }
      below = prev;
    }
  }
  if (ursn_cluster_vertices_scratch_bytes(0, 1, 1) || ursn_cluster_vertices_scratch_bytes(65536, 1, 1) ||
      ursn_cluster_vertices_scratch_bytes(1, -1, 1) || ursn_cluster_vertices_scratch_bytes(1, (int64_t)1 << 30, 1) ||
      ursn_cluster_vertices_scratch_bytes(1, 1, -1) || ursn_cluster_vertices_scratch_bytes(1, 1, (int64_t)1 << 30) ||
      ursn_cluster_vertices_scratch_bytes(INT32_MIN, INT64_MIN, INT64_MIN) || ursn_cluster_vertices_scratch_bytes(1, INT64_MAX, INT64_MAX)) {
    printf("FAILED: the query answers outside its domain\n");
    ++failures;
  }
  if (launches) { printf("FAILED: %ld launches noted\n", launches); ++failures; }
  printf("%ld refused, %ld launches\n", refused, launches);
  printf(failures ? "FAILED: %ld\n" : "argument checks consistent\n", failures);
  return failures != 0;
}
