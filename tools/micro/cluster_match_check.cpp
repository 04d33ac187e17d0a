// Host-side check of ursn_cluster_match's argument checks and scratch query: a stand-alone program that links cluster_match.hip
// alone (the two library hooks it needs are defined here) and makes only calls that are refused before any launch, with fake
// device pointers, so it needs no GPU.  Meant to be built with the sanitizers on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         u-resnet_amd/csrc/cluster_match.hip tools/micro/cluster_match_check.cpp -o cluster_match_check && ./cluster_match_check
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
  ursn_cluster_match_desc d;
  ursn_cluster_match_out o;
  void* scratch;
  size_t bytes;
};

static Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.d.n = 2, c.d.m_total = 10;
  c.d.offsets = (const int64_t*)fake(0), c.d.cluster_a = (const int32_t*)fake(0x1000), c.d.table_offsets_a = (const int64_t*)fake(0x2000);
  c.d.cluster_b = (const int32_t*)fake(0x3000), c.d.table_offsets_b = (const int64_t*)fake(0x4000), c.d.value = (const float*)fake(0x5000);
  c.o.a_int = (int64_t*)fake(0x10000), c.o.a_real = (double*)fake(0x11000), c.o.cap_a = 10;
  c.o.b_int = (int64_t*)fake(0x12000), c.o.b_real = (double*)fake(0x13000), c.o.cap_b = 10;
  c.o.event_int = (int64_t*)fake(0x14000), c.o.event_real = (double*)fake(0x15000);
  c.o.pair_offsets = (int64_t*)fake(0x16000), c.o.pair_b = (int32_t*)fake(0x17000), c.o.pair_n = (int64_t*)fake(0x18000);
  c.o.pair_q = (int64_t*)fake(0x19000), c.o.pair_cap = 10, c.o.status = (int32_t*)fake(0x1a000);
  c.scratch = fake(0x40000), c.bytes = 0;   // 0 bytes: whatever passes every other check is refused by the last one
  return c;
}

static void expect(const Case& c, const char* text) {
  g_err[0] = 0;
  const int rc = ursn_cluster_match(&c.d, &c.o, c.scratch, c.bytes, nullptr);
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
  { g_err[0] = 0; if (ursn_cluster_match(nullptr, &c.o, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  { g_err[0] = 0; if (ursn_cluster_match(&c.d, nullptr, c.scratch, 0, nullptr) == 0) ++failures; else ++refused; }
  for (int n : {0, -1, 65536, INT32_MAX, INT32_MIN}) { Case k = good(); k.d.n = n; expect(k, "outside [1, 65535]"); }
  for (int64_t m : {(int64_t)-1, (int64_t)1 << 31, INT64_MAX, INT64_MIN}) { Case k = good(); k.d.m_total = m; expect(k, "outside [0, 2^31)"); }
  for (int64_t cap : {(int64_t)-1, INT64_MIN}) {
    { Case k = good(); k.o.cap_a = cap; expect(k, "cap_a = "); }
    { Case k = good(); k.o.cap_b = cap; expect(k, "cap_b = "); }
    { Case k = good(); k.o.pair_cap = cap; expect(k, "pair_cap = "); }
  }
  { Case k = good(); k.d.offsets = nullptr; expect(k, "null offsets / table_offsets_a / table_offsets_b"); }
  { Case k = good(); k.d.table_offsets_a = nullptr; expect(k, "null offsets / table_offsets_a / table_offsets_b"); }
  { Case k = good(); k.d.table_offsets_b = nullptr; expect(k, "null offsets / table_offsets_a / table_offsets_b"); }
  { Case k = good(); k.d.cluster_a = nullptr; expect(k, "null cluster_a / cluster_b"); }
  { Case k = good(); k.d.cluster_b = nullptr; expect(k, "null cluster_a / cluster_b"); }
  { Case k = good(); k.o.status = nullptr; expect(k, "null out->status"); }
  { Case k = good(); k.o.event_int = nullptr; expect(k, "null out->event_int / out->event_real"); }
  { Case k = good(); k.o.event_real = nullptr; expect(k, "null out->event_int / out->event_real"); }
  { Case k = good(); k.o.a_int = nullptr; expect(k, "null out->a_int / out->a_real"); }
  { Case k = good(); k.o.a_real = nullptr; expect(k, "null out->a_int / out->a_real"); }
  { Case k = good(); k.o.b_int = nullptr; expect(k, "null out->b_int / out->b_real"); }
  { Case k = good(); k.o.b_real = nullptr; expect(k, "null out->b_int / out->b_real"); }
  { Case k = good(); k.o.pair_b = nullptr; expect(k, "together or not at all"); }
  { Case k = good(); k.o.pair_n = nullptr; expect(k, "together or not at all"); }
  { Case k = good(); k.o.pair_q = nullptr; expect(k, "together or not at all"); }
  { Case k = good(); k.o.pair_b = nullptr; k.o.pair_q = nullptr; expect(k, "together or not at all"); }
  { Case k = good(); k.o.pair_offsets = nullptr; expect(k, "need out->pair_offsets"); }
  { Case k = good(); k.scratch = nullptr; expect(k, "null scratch"); }
  // legal: no values; counts only; no cell list; no rows wanted; no entries; the largest caps
  { Case k = good(); k.d.value = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.pair_b = nullptr; k.o.pair_n = nullptr; k.o.pair_q = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.pair_b = nullptr; k.o.pair_n = nullptr; k.o.pair_q = nullptr; k.o.pair_offsets = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_a = k.o.cap_b = 0; k.o.a_int = k.o.b_int = nullptr; k.o.a_real = k.o.b_real = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.m_total = 0; k.d.cluster_a = k.d.cluster_b = nullptr; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.o.cap_a = k.o.cap_b = k.o.pair_cap = INT64_MAX; expect(k, "scratch of 0 bytes"); }
  { Case k = good(); k.d.offsets = (const int64_t*)fake(4); expect(k, "8-byte aligned"); }
  { Case k = good(); k.d.table_offsets_b = (const int64_t*)fake(0x4004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.o.a_int = (int64_t*)fake(0x10004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.o.b_real = (double*)fake(0x13004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.o.event_real = (double*)fake(0x15004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.o.pair_offsets = (int64_t*)fake(0x16004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.o.pair_q = (int64_t*)fake(0x19004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.scratch = fake(0x40004); expect(k, "8-byte aligned"); }
  { Case k = good(); k.d.cluster_a = (const int32_t*)fake(0x1002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.d.value = (const float*)fake(0x5002); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.pair_b = (int32_t*)fake(0x17001); expect(k, "4-byte aligned"); }
  { Case k = good(); k.o.status = (int32_t*)fake(0x1a001); expect(k, "4-byte aligned"); }
  // the query: 0 outside the domain; inside it at least 8, 8-byte granular, monotone in the list length; 8 short is refused
  const int64_t ms[] = {0, 1, 2, 3, 255, 256, 2047, 2048, 2049, 1000000, ((int64_t)1 << 31) - 1};
  for (int n : {1, 2, 65535}) {
    size_t prev = 0;
    for (int64_t m : ms) {
      const size_t b = ursn_cluster_match_scratch_bytes(n, m, m, m, m);
      if (b < 8 || b % 8 != 0 || b < prev || b < (size_t)m * 48) { printf("FAILED: query(%d, %lld) = %zu\n", n, (long long)m, b); ++failures; }
      prev = b;
      Case k = good();
      k.d.n = n, k.d.m_total = m, k.o.cap_a = k.o.cap_b = k.o.pair_cap = m, k.bytes = b - 8;
      expect(k, "is too small");
    }
  }
  if (ursn_cluster_match_scratch_bytes(0, 1, 1, 1, 1) || ursn_cluster_match_scratch_bytes(65536, 1, 1, 1, 1) ||
      ursn_cluster_match_scratch_bytes(1, -1, 1, 1, 1) || ursn_cluster_match_scratch_bytes(1, (int64_t)1 << 31, 1, 1, 1) ||
      ursn_cluster_match_scratch_bytes(1, 1, -1, 1, 1) || ursn_cluster_match_scratch_bytes(1, 1, 1, -1, 1) ||
      ursn_cluster_match_scratch_bytes(1, 1, 1, 1, -1) || ursn_cluster_match_scratch_bytes(1, INT64_MAX, INT64_MAX, 1, 1)) {
    printf("FAILED: the query answers outside its domain\n");
    ++failures;
  }
  if (launches) { printf("FAILED: %ld launches noted\n", launches); ++failures; }
  printf("%ld refused, %ld launches\n", refused, launches);
  printf(failures ? "FAILED: %ld\n" : "argument checks consistent\n", failures);
  return failures != 0;
}
