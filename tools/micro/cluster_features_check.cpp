// Host-side check of ursn_cluster_features' argument checks and scratch query: a stand-alone program that links
// cluster_features.hip alone (the two library hooks it needs are defined here) and makes only calls that are refused before any
// launch, with fake device pointers, so it needs no GPU.  Meant to be built with the sanitizers on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/cluster_features.hip tools/micro/cluster_features_check.cpp -o cluster_features_check && ./cluster_features_check
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
  ursn_cluster_feat_desc d;
  ursn_cluster_feat_out o;
  void* scratch;
  size_t bytes;
};

static Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.d.ndim = 3, c.d.spatial[0] = c.d.spatial[1] = c.d.spatial[2] = 8, c.d.n = 2, c.d.m_total = 10;
  c.d.offsets = (const int64_t*)fake(0), c.d.index = (const int32_t*)fake(0x1000), c.d.value = (const float*)fake(0x2000);
  c.d.cluster = (const int32_t*)fake(0x3000), c.d.table_offsets = (const int64_t*)fake(0x4000);
  c.o.itab = (int64_t*)fake(0x10000), c.o.rtab = (double*)fake(0x20000), c.o.cap = 10, c.o.status = (int32_t*)fake(0x30000);
  c.scratch = fake(0x40000), c.bytes = 0;   // 0 bytes: whatever passes every other check is refused by the last one
  return c;
}

static void expect(const Case& c, const char* text) {
  g_err[0] = 0;
  const int rc = ursn_cluster_features(&c.d, &c.o, c.scratch, c.bytes, nullptr);
  if (rc == 0 || !strstr(g_err, text)) {
    printf("FAILED: expected \"%s\", got rc %d \"%s\"\n", text, rc, g_err);
    ++failures;
  } else {
    ++refused;
  }
}

int main() {
  Case c = good();
  expect(c, "scratch of 0 bytes is too small");
  { g_err[0] = 0; if (ursn_cluster_features(nullptr, &c.o, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  { g_err[0] = 0; if (ursn_cluster_features(&c.d, nullptr, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  for (int nd : {-1, 0, 1, 4, 1 << 30}) { Case k = good(); k.d.ndim = nd; expect(k, "must be 2 or 3"); }
  for (int ax = 0; ax < 3; ++ax)
    for (int e : {0, -1, 32769, INT32_MIN, INT32_MAX}) { Case k = good(); k.d.spatial[ax] = e; expect(k, "outside [1, 32768]"); }
  { Case k = good(); k.d.spatial[0] = k.d.spatial[1] = 32768; k.d.spatial[2] = 2; expect(k, "prod(spatial) >= 2^31"); }
  { Case k = good(); k.d.spatial[0] = k.d.spatial[1] = k.d.spatial[2] = 32768; expect(k, "prod(spatial) >= 2^31"); }   // 2^45: no overflow
  { Case k = good(); k.d.spatial[0] = 32768; k.d.spatial[1] = k.d.spatial[2] = 2; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.ndim = 2; k.d.spatial[0] = k.d.spatial[1] = 32768; k.d.spatial[2] = -7; expect(k, "scratch of 0 bytes"); }
  for (int n : {0, -1, 65536, INT32_MAX}) { Case k = good(); k.d.n = n; expect(k, "outside [1, 65535]"); }
  for (int64_t m : {(int64_t)-1, (int64_t)1 << 31, INT64_MAX, INT64_MIN}) { Case k = good(); k.d.m_total = m; expect(k, "outside [0, 2^31)"); }
  for (int64_t cap : {(int64_t)-1, INT64_MIN}) { Case k = good(); k.o.cap = cap; expect(k, "cap = "); }
  { Case k = good(); k.d.offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.table_offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.index = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.d.cluster = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.o.status = nullptr; expect(k, "null out->status"); }
  { Case k = good(); k.o.itab = nullptr; expect(k, "null out->itab / out->rtab"); }
  { Case k = good(); k.o.rtab = nullptr; expect(k, "null out->itab / out->rtab"); }
  { Case k = good(); k.scratch = nullptr; expect(k, "null scratch"); }
  { Case k = good(); k.d.value = nullptr; expect(k, "scratch of 0 bytes"); }                       // legal: no charge
  { Case k = good(); k.o.cap = INT64_MAX; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.offsets = (const int64_t*)fake(4); expect(k, "8-byte aligned"); }
  { Case k = good(); k.o.itab = (int64_t*)fake(0x10004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.scratch = fake(0x40004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.d.value = (const float*)fake(0x2002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.status = (int32_t*)fake(0x30001); expect(k, "4-byte aligned"); }
  // the query: 0 outside the domain; inside it at least 8, 8-byte granular, monotone in the list length; 8 short is refused
  const int64_t ms[] = {0, 1, 2, 3, 255, 256, 2047, 2048, 2049, 1000000, ((int64_t)1 << 31) - 1};
  for (int n : {1, 2, 65535}) {
    size_t prev = 0;
    for (int64_t m : ms) {
      const size_t b = ursn_cluster_features_scratch_bytes(n, m, m);
      if (b < 8 || b % 8 != 0 || b < prev || b < (size_t)m * 4) { printf("FAILED: query(%d, %lld) = %zu\n", n, (long long)m, b); ++failures; }
      prev = b;
      Case k = good();
      k.d.n = n, k.d.m_total = m, k.o.cap = m, k.bytes = b - 8;
      expect(k, "is too small");
    }
  }
  if (ursn_cluster_features_scratch_bytes(0, 1, 1) || ursn_cluster_features_scratch_bytes(65536, 1, 1) ||
      ursn_cluster_features_scratch_bytes(1, -1, 1) || ursn_cluster_features_scratch_bytes(1, (int64_t)1 << 31, 1) ||
      ursn_cluster_features_scratch_bytes(1, 1, -1) || ursn_cluster_features_scratch_bytes(1, INT64_MAX, INT64_MAX)) {
    printf("FAILED: the query answers outside its domain\n");
    ++failures;
  }
  if (launches) { printf("FAILED: %ld launches noted\n", launches); ++failures; }
  printf("%ld refused, %ld launches\n", refused, launches);
  printf(failures ? "FAILED: %ld\n" : "argument checks consistent\n", failures);
  return failures != 0;
}
