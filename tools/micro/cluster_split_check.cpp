// Host-side check of ursn_cluster_split's argument checks and scratch query: a stand-alone program that links cluster_split.hip
// alone (the two library hooks it needs are defined here) and makes only calls that are refused before any launch, with fake
// device pointers, so it needs no GPU.  Meant to be built with the sanitizers on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/cluster_split.hip tools/micro/cluster_split_check.cpp -o cluster_split_check && ./cluster_split_check
#include <math.h>
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
  ursn_cluster_split_desc d;
  ursn_cluster_split_out o;
  void* scratch;
  size_t bytes;
};

static Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.d.ndim = 3, c.d.spatial[0] = 7, c.d.spatial[1] = 9, c.d.spatial[2] = 11, c.d.n = 2, c.d.radius = 2, c.d.m_total = 10;
  c.d.offsets = (const int64_t*)fake(0), c.d.index = (const int32_t*)fake(0x1000), c.d.cluster = (const int32_t*)fake(0x2000);
  c.d.table_offsets = (const int64_t*)fake(0x3000), c.d.size = (const int32_t*)fake(0x5000), c.d.cls = (const uint8_t*)fake(0x7000);
  c.d.kink_cos = -0.7, c.d.min_size = 8, c.d.class_mask = 6, c.d.grow = 4;
  c.o.split = (int32_t*)fake(0x10000), c.o.mark = (uint8_t*)fake(0x11000), c.o.piece_offsets = (int64_t*)fake(0x12000);
  c.o.first = (int32_t*)fake(0x13000), c.o.size = (int32_t*)fake(0x14000), c.o.cls = (uint8_t*)fake(0x15000);
  c.o.piece_itab = (int64_t*)fake(0x16000), c.o.cap_pieces = 10, c.o.junction_offsets = (int64_t*)fake(0x17000);
  c.o.junction_itab = (int64_t*)fake(0x18000), c.o.junction_rtab = (double*)fake(0x19000), c.o.cap_junctions = 10;
  c.o.rows = (int32_t*)fake(0x1a000), c.o.cap_rows = 10, c.o.event = (int64_t*)fake(0x1d000), c.o.status = (int32_t*)fake(0x1e000);
  c.scratch = fake(0x40000), c.bytes = 0;   // 0 bytes: whatever passes every other check is refused by the last one
  return c;
}

static void expect(const Case& c, const char* text) {
  g_err[0] = 0;
  const int rc = ursn_cluster_split(&c.d, &c.o, c.scratch, c.bytes, nullptr);
  if (rc == 0 || strncmp(g_err, "cluster_split:", 14) != 0 || !strstr(g_err, text)) {
    printf("FAILED: expected \"%s\", got rc %d \"%s\"\n", text, rc, g_err);
    ++failures;
  } else {
    ++refused;
  }
}

int main() {
  Case c = good();
  expect(c, "scratch of 0 bytes is too small");
  { g_err[0] = 0; if (ursn_cluster_split(nullptr, &c.o, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  { g_err[0] = 0; if (ursn_cluster_split(&c.d, nullptr, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
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
  for (double kc : {-1.1, 1.5, -1e300, 1e300, (double)NAN, (double)INFINITY, -(double)INFINITY, 1.0000000000000002, -1.0000000000000002}) {
    Case k = good(); k.d.kink_cos = kc; expect(k, "outside [-1, 1]");
  }
  for (int s : {0, -1, INT32_MIN}) { Case k = good(); k.d.min_size = s; expect(k, "min_size = "); }
  for (int g : {-1, 9, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.grow = g; expect(k, "outside [0, 8]"); }
  for (int v : {1, -1, INT32_MIN}) { Case k = good(); k.d.reserved = v; expect(k, "reserved = "); }
  for (int64_t cap : {(int64_t)-1, INT64_MIN}) {
    { Case k = good(); k.o.cap_rows = cap; expect(k, "cap_rows = "); }
    { Case k = good(); k.o.cap_pieces = cap; expect(k, "cap_pieces = "); }
    { Case k = good(); k.o.cap_junctions = cap; expect(k, "cap_junctions = "); }
  }
  { Case k = good(); k.d.offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.table_offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.index = nullptr; expect(k, "null index / cluster / size"); }
  { Case k = good(); k.d.cluster = nullptr; expect(k, "null index / cluster / size"); }
  { Case k = good(); k.d.size = nullptr; expect(k, "null index / cluster / size"); }
  for (uint32_t mask : {1u, 6u, 0x80000000u, 0xFFFFFFFFu}) { Case k = good(); k.d.cls = nullptr; k.d.class_mask = mask; expect(k, "needs cls"); }
  { Case k = good(); k.o.status = nullptr; expect(k, "null out->status"); }
  { Case k = good(); k.o.piece_offsets = nullptr; expect(k, "null out->piece_offsets / out->junction_offsets / out->event"); }
  { Case k = good(); k.o.junction_offsets = nullptr; expect(k, "null out->piece_offsets / out->junction_offsets / out->event"); }
  { Case k = good(); k.o.event = nullptr; expect(k, "null out->piece_offsets / out->junction_offsets / out->event"); }
  { Case k = good(); k.o.split = nullptr; expect(k, "null out->split / out->mark"); }
  { Case k = good(); k.o.mark = nullptr; expect(k, "null out->split / out->mark"); }
  { Case k = good(); k.o.piece_itab = nullptr; expect(k, "null out->piece_itab"); }
  { Case k = good(); k.o.first = nullptr; expect(k, "null out->piece_itab"); }
  { Case k = good(); k.o.size = nullptr; expect(k, "null out->piece_itab"); }
  { Case k = good(); k.o.cls = nullptr; expect(k, "null out->piece_itab"); }
  { Case k = good(); k.o.junction_itab = nullptr; expect(k, "null out->junction_itab / out->junction_rtab"); }
  { Case k = good(); k.o.junction_rtab = nullptr; expect(k, "null out->junction_itab / out->junction_rtab"); }
  { Case k = good(); k.o.rows = nullptr; expect(k, "null out->rows"); }
  { Case k = good(); k.scratch = nullptr; expect(k, "null scratch"); }
  // legal: no cls; cls and mark at odd addresses; 2-D at the largest extents; the ends of every range; no rows, pieces or junctions;
  // no entries; the largest caps
  { Case k = good(); k.d.cls = nullptr; k.d.class_mask = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.cls = (const uint8_t*)fake(0x7003); k.d.class_mask = 0xFFFFFFFFu; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cls = (uint8_t*)fake(0x15003); k.o.mark = (uint8_t*)fake(0x11001); expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.ndim = 2; k.d.spatial[0] = k.d.spatial[1] = 32768; k.d.spatial[2] = INT32_MIN; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.radius = 1, k.d.min_size = 1, k.d.kink_cos = -1.0, k.d.grow = 0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.radius = 3, k.d.min_size = INT32_MAX, k.d.kink_cos = 1.0, k.d.grow = 8; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.kink_cos = -0.0; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = 0; k.o.rows = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_pieces = 0; k.o.piece_itab = nullptr; k.o.first = k.o.size = nullptr; k.o.cls = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_junctions = 0; k.o.junction_itab = nullptr; k.o.junction_rtab = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.m_total = 0; k.d.index = k.d.cluster = k.d.size = nullptr; k.o.split = nullptr; k.o.mark = nullptr;
    expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = k.o.cap_pieces = k.o.cap_junctions = INT64_MAX; k.d.m_total = ((int64_t)1 << 30) - 1;
    expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.offsets = (const int64_t*)fake(4); expect(k, "8-byte"); }
  { Case k = good(); k.d.table_offsets = (const int64_t*)fake(0x3004); expect(k, "8-byte"); }
  { Case k = good(); k.o.piece_offsets = (int64_t*)fake(0x12004); expect(k, "8-byte"); }
  { Case k = good(); k.o.piece_itab = (int64_t*)fake(0x16004); expect(k, "8-byte"); }
  { Case k = good(); k.o.junction_offsets = (int64_t*)fake(0x17004); expect(k, "8-byte"); }
  { Case k = good(); k.o.junction_itab = (int64_t*)fake(0x18004); expect(k, "8-byte"); }
  { Case k = good(); k.o.junction_rtab = (double*)fake(0x19004); expect(k, "8-byte"); }
  { Case k = good(); k.o.event = (int64_t*)fake(0x1d004); expect(k, "8-byte"); }
  { Case k = good(); k.scratch = fake(0x40004); expect(k, "8-byte"); }
  { Case k = good(); k.d.index = (const int32_t*)fake(0x1002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.cluster = (const int32_t*)fake(0x2001); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.size = (const int32_t*)fake(0x5002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.split = (int32_t*)fake(0x10002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.first = (int32_t*)fake(0x13002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.size = (int32_t*)fake(0x14001); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.rows = (int32_t*)fake(0x1a002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.status = (int32_t*)fake(0x1e001); expect(k, "4-byte aligned"); }
  // the query: 0 outside the domain; inside it at least 8, 8-byte granular, monotone in the list length, room for the two accumulator
  // tables (48 + 128 bytes per entry) and the fourteen int32 words per entry; 8 short is refused
  const int64_t ms[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 2047, 2048, 2049, 1000000, ((int64_t)1 << 30) - 1};
  for (int n : {1, 2, 65535}) {
    size_t prev = 0;
    for (int64_t m : ms) {
      const size_t b = ursn_cluster_split_scratch_bytes(n, m);
      if (b < 8 || b % 8 != 0 || b < prev || b < (size_t)m * 232 + (size_t)n * 16) {
        printf("FAILED: query(%d, %lld) = %zu\n", n, (long long)m, b);
        ++failures;
      }
      prev = b;
      Case k = good();
      k.d.n = n, k.d.m_total = m, k.bytes = b - 8;
      expect(k, "is too small");
    }
  }
  if (ursn_cluster_split_scratch_bytes(0, 1) || ursn_cluster_split_scratch_bytes(65536, 1) || ursn_cluster_split_scratch_bytes(1, -1) ||
      ursn_cluster_split_scratch_bytes(1, (int64_t)1 << 30) || ursn_cluster_split_scratch_bytes(INT32_MIN, INT64_MIN) ||
      ursn_cluster_split_scratch_bytes(1, INT64_MAX)) {
    printf("FAILED: the query answers outside its domain\n");
    ++failures;
  }
  if (launches) { printf("FAILED: %ld launches noted\n", launches); ++failures; }
  printf("%ld refused, %ld launches\n", refused, launches);
  printf(failures ? "FAILED: %ld\n" : "argument checks consistent\n", failures);
  return failures != 0;
}
