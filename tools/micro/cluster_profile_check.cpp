// Host-side check of ursn_cluster_profile's argument checks and scratch query: a stand-alone program that links cluster_profile.hip
// alone (the two library hooks it needs are defined here) and makes only calls that are refused before any launch, with fake
// device pointers, so it needs no GPU.  Meant to be built with the sanitizers on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/cluster_profile.hip tools/micro/cluster_profile_check.cpp -o cluster_profile_check && ./cluster_profile_check
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
  ursn_cluster_prof_desc d;
  ursn_cluster_prof_out o;
  void* scratch;
  size_t bytes;
};

static Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.d.ndim = 3, c.d.spatial[0] = 7, c.d.spatial[1] = 9, c.d.spatial[2] = 11, c.d.n = 2, c.d.m_total = 10;
  c.d.offsets = (const int64_t*)fake(0), c.d.index = (const int32_t*)fake(0x1000), c.d.value = (const float*)fake(0x4000);
  c.d.cluster = (const int32_t*)fake(0x2000), c.d.table_offsets = (const int64_t*)fake(0x3000);
  c.d.itab = (const int64_t*)fake(0x5000), c.d.rtab = (const double*)fake(0x6000), c.d.feat_cap = 10;
  c.d.step = 1.0, c.d.end_bins = 3, c.d.max_bins = 4096;
  c.o.bin_offsets = (int64_t*)fake(0x10000), c.o.bin_itab = (int64_t*)fake(0x11000), c.o.bin_rtab = (double*)fake(0x12000);
  c.o.row_itab = (int64_t*)fake(0x13000), c.o.row_rtab = (double*)fake(0x14000), c.o.cap_rows = 10, c.o.bin_cap = 64;
  c.o.status = (int32_t*)fake(0x17000);
  c.scratch = fake(0x40000), c.bytes = 0;   // 0 bytes: whatever passes every other check is refused by the last one
  return c;
}

static void expect(const Case& c, const char* text) {
  g_err[0] = 0;
  const int rc = ursn_cluster_profile(&c.d, &c.o, c.scratch, c.bytes, nullptr);
  if (rc == 0 || strncmp(g_err, "cluster_profile:", 16) != 0 || !strstr(g_err, text)) {
    printf("FAILED: expected \"%s\", got rc %d \"%s\"\n", text, rc, g_err);
    ++failures;
  } else {
    ++refused;
  }
}

int main() {
  Case c = good();
  expect(c, "scratch of 0 bytes is too small");
  { g_err[0] = 0; if (ursn_cluster_profile(nullptr, &c.o, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  { g_err[0] = 0; if (ursn_cluster_profile(&c.d, nullptr, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  for (int n : {0, -1, 65536, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.n = n; expect(k, "outside [1, 65535]"); }
  for (int64_t m : {(int64_t)-1, (int64_t)1 << 31, INT64_MAX, INT64_MIN}) { Case k = good(); k.d.m_total = m; expect(k, "outside [0, 2^31)"); }
  for (int nd : {0, 1, 4, -3, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.ndim = nd; expect(k, "must be 2 or 3"); }
  for (int s : {0, -1, 32769, INT32_MAX, INT32_MIN}) {
    for (int ax = 0; ax < 3; ++ax) { Case k = good(); k.d.spatial[ax] = s; expect(k, "outside [1, 32768]"); }
  }
  { Case k = good(); k.d.spatial[0] = k.d.spatial[1] = k.d.spatial[2] = 32768; expect(k, "prod(spatial) >= 2^31"); }
  { Case k = good(); k.d.spatial[0] = 2048, k.d.spatial[1] = 1024, k.d.spatial[2] = 1024; expect(k, "prod(spatial) >= 2^31"); }
  for (double s : {0.0, 0.4999999, -1.0, 4096.5, (double)INFINITY, -(double)INFINITY, (double)NAN, 1e300}) {
    Case k = good(); k.d.step = s; expect(k, "outside [0.5, 4096]");
  }
  for (int e : {0, 17, -1, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.end_bins = e; expect(k, "end_bins = "); }
  for (int b : {0, 65537, -1, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.max_bins = b; expect(k, "max_bins = "); }
  for (int64_t cap : {(int64_t)-1, INT64_MIN}) {
    { Case k = good(); k.o.cap_rows = cap; expect(k, "cap_rows = "); }
    { Case k = good(); k.d.feat_cap = cap; expect(k, "feat_cap = "); }
  }
  for (int64_t cap : {(int64_t)-1, (int64_t)1 << 31, INT64_MAX, INT64_MIN}) { Case k = good(); k.o.bin_cap = cap; expect(k, "bin_cap = "); }
  { Case k = good(); k.d.offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.table_offsets = nullptr; expect(k, "null offsets / table_offsets"); }
  { Case k = good(); k.d.index = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.d.cluster = nullptr; expect(k, "null index / cluster"); }
  { Case k = good(); k.d.itab = nullptr; expect(k, "null itab / rtab"); }
  { Case k = good(); k.d.rtab = nullptr; expect(k, "null itab / rtab"); }
  { Case k = good(); k.o.status = nullptr; expect(k, "null out->status / out->bin_offsets"); }
  { Case k = good(); k.o.bin_offsets = nullptr; expect(k, "null out->status / out->bin_offsets"); }
  { Case k = good(); k.o.row_itab = nullptr; expect(k, "null out->row_itab / out->row_rtab"); }
  { Case k = good(); k.o.row_rtab = nullptr; expect(k, "null out->row_itab / out->row_rtab"); }
  { Case k = good(); k.o.bin_itab = nullptr; expect(k, "null out->bin_itab / out->bin_rtab"); }
  { Case k = good(); k.o.bin_rtab = nullptr; expect(k, "null out->bin_itab / out->bin_rtab"); }
  { Case k = good(); k.scratch = nullptr; expect(k, "null scratch"); }
  // legal: no values; 2-D at the largest extents; the ends of every range; no rows, bins or object records; no entries
  { Case k = good(); k.d.value = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.ndim = 2; k.d.spatial[0] = k.d.spatial[1] = 32768; k.d.spatial[2] = INT32_MIN; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.step = 0.5, k.d.end_bins = 1, k.d.max_bins = 1; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.step = 4096.0, k.d.end_bins = 16, k.d.max_bins = 65536; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = 0; k.o.row_itab = nullptr; k.o.row_rtab = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.bin_cap = 0; k.o.bin_itab = nullptr; k.o.bin_rtab = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.feat_cap = 0; k.d.itab = nullptr; k.d.rtab = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.m_total = 0; k.d.index = k.d.cluster = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_rows = k.d.feat_cap = INT64_MAX; k.o.bin_cap = ((int64_t)1 << 31) - 1; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.offsets = (const int64_t*)fake(4); expect(k, "8-byte"); }
  { Case k = good(); k.d.table_offsets = (const int64_t*)fake(0x3004); expect(k, "8-byte"); }
  { Case k = good(); k.d.itab = (const int64_t*)fake(0x5004); expect(k, "8-byte"); }
  { Case k = good(); k.d.rtab = (const double*)fake(0x6004); expect(k, "8-byte"); }
  { Case k = good(); k.o.bin_offsets = (int64_t*)fake(0x10004); expect(k, "8-byte"); }
  { Case k = good(); k.o.bin_itab = (int64_t*)fake(0x11004); expect(k, "8-byte"); }
  { Case k = good(); k.o.bin_rtab = (double*)fake(0x12004); expect(k, "8-byte"); }
  { Case k = good(); k.o.row_itab = (int64_t*)fake(0x13004); expect(k, "8-byte"); }
  { Case k = good(); k.o.row_rtab = (double*)fake(0x14004); expect(k, "8-byte"); }
  { Case k = good(); k.scratch = fake(0x40004); expect(k, "8-byte"); }
  { Case k = good(); k.d.index = (const int32_t*)fake(0x1002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.cluster = (const int32_t*)fake(0x2001); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.value = (const float*)fake(0x4002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.status = (int32_t*)fake(0x17001); expect(k, "4-byte aligned"); }
  // the query: 0 outside the domain; inside it at least 8, 8-byte granular, monotone in the list length and the row cap, room for
  // 12 bytes per considered row; 8 short is refused
  const int64_t ms[] = {0, 1, 2, 3, 255, 256, 2047, 2048, 2049, 1000000, ((int64_t)1 << 31) - 1};
  for (int n : {1, 2, 65535}) {
    for (int64_t bc : {(int64_t)0, (int64_t)1000, ((int64_t)1 << 31) - 1}) {
      size_t prev = 0;
      for (int64_t m : ms) {
        const size_t b = ursn_cluster_profile_scratch_bytes(n, m, m, bc);
        const size_t half = ursn_cluster_profile_scratch_bytes(n, m, m / 2, bc);
        if (b < 8 || b % 8 != 0 || b < prev || b < (size_t)m * 12 || half > b || half < (size_t)(m / 2) * 12 ||
            ursn_cluster_profile_scratch_bytes(n, m, INT64_MAX, bc) != b) {
          printf("FAILED: query(%d, %lld, %lld) = %zu\n", n, (long long)m, (long long)bc, b);
          ++failures;
        }
        prev = b;
        Case k = good();
        k.d.n = n, k.d.m_total = m, k.o.cap_rows = m, k.o.bin_cap = bc, k.bytes = b - 8;
        expect(k, "is too small");
      }
    }
  }
  if (ursn_cluster_profile_scratch_bytes(0, 1, 1, 1) || ursn_cluster_profile_scratch_bytes(65536, 1, 1, 1) ||
      ursn_cluster_profile_scratch_bytes(1, -1, 1, 1) || ursn_cluster_profile_scratch_bytes(1, (int64_t)1 << 31, 1, 1) ||
      ursn_cluster_profile_scratch_bytes(1, 1, -1, 1) || ursn_cluster_profile_scratch_bytes(1, 1, 1, -1) ||
      ursn_cluster_profile_scratch_bytes(1, 1, 1, (int64_t)1 << 31) ||
      ursn_cluster_profile_scratch_bytes(INT32_MIN, INT64_MIN, INT64_MIN, INT64_MIN)) {
    printf("FAILED: the query answers outside its domain\n");
    ++failures;
  }
  if (launches) { printf("FAILED: %ld launches noted\n", launches); ++failures; }
  printf("%ld refused, %ld launches\n", refused, launches);
  printf(failures ? "FAILED: %ld\n" : "argument checks consistent\n", failures);
  return failures != 0;
}
