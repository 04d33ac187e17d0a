// Host-side memory check of ursn_normalize_weights' argument handling: a stand-alone program that links weight_norm.hip alone
// (the three library hooks it needs are defined here), calls the scratch query and every refusal path -- all of which return
// before any device call -- and is meant to be built with AddressSanitizer on the host side:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address \
//         u-resnet_amd/csrc/weight_norm.hip tools/micro/wnorm_refusals.cpp -o wnorm_refusals && ./wnorm_refusals
#include <stdarg.h>
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
void ursn_note_kernel(const char*) {}

static int failures = 0;
static void refused(const char* what, int rc, const char* text) {
  const bool ok = rc != 0 && strstr(g_err, text) != nullptr;
  printf("%-28s rc %d  %s  [%s]\n", what, rc, ok ? "ok" : "UNEXPECTED", g_err);
  failures += !ok;
  g_err[0] = 0;
}

int main() {
  float* const W = (float*)0x10000;
  float* const O = (float*)0x110000;
  void* const S = (void*)0x210000;
  const size_t big = 1 << 20;
  if (ursn_normalize_weights_scratch_bytes(2, 64) != 16 || ursn_normalize_weights_scratch_bytes(0, 64) != 0 ||
      ursn_normalize_weights_scratch_bytes(1, (int64_t)1 << 31) != 0 || ursn_normalize_weights_scratch_bytes(65536, 1) != 0) {
    printf("scratch query UNEXPECTED\n");
    ++failures;
  }
  refused("null weight", ursn_normalize_weights(nullptr, O, 2, 64, nullptr, S, big, nullptr), "null");
  refused("null out", ursn_normalize_weights(W, nullptr, 2, 64, nullptr, S, big, nullptr), "null");
  refused("null scratch", ursn_normalize_weights(W, O, 2, 64, nullptr, nullptr, big, nullptr), "null");
  refused("n = 0", ursn_normalize_weights(W, O, 0, 64, nullptr, S, big, nullptr), "outside [1, 65535]");
  refused("n = 65536", ursn_normalize_weights(W, O, 65536, 64, nullptr, S, big, nullptr), "outside [1, 65535]");
  refused("voxels = 0", ursn_normalize_weights(W, O, 2, 0, nullptr, S, big, nullptr), "< 1");
  refused("voxels = 2^31", ursn_normalize_weights(W, O, 2, (int64_t)1 << 31, nullptr, S, big, nullptr), ">= 2^31");
  refused("scratch too small", ursn_normalize_weights(W, O, 2, 64, nullptr, S, 15, nullptr), "too small");
  refused("scratch misaligned", ursn_normalize_weights(W, O, 2, 64, nullptr, (char*)S + 4, big, nullptr), "8-byte aligned");
  refused("weight misaligned", ursn_normalize_weights((float*)((char*)W + 2), O, 2, 64, nullptr, S, big, nullptr), "4-byte aligned");
  refused("out misaligned", ursn_normalize_weights(W, (float*)((char*)O + 1), 2, 64, nullptr, S, big, nullptr), "4-byte aligned");
  refused("partial overlap", ursn_normalize_weights(W, W + 1, 2, 64, nullptr, S, big, nullptr), "overlaps");
  refused("overlap from below", ursn_normalize_weights(W + 127, W, 2, 64, nullptr, S, big, nullptr), "overlaps");
  printf(failures ? "FAILED: %d\n" : "all refusals as expected\n", failures);
  return failures != 0;
}
