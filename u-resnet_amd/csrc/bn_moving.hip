// BatchNorm moving statistics (gfx950): the half of slim.batch_norm the reference never runs (is_training stays True and nothing
// runs UPDATE_OPS).  Two tiny launches over per-channel vectors, each ONE launch for every layer of a
// plan (grid.y = layer, read from a device table of the layers' statistics vectors), no atomics, nothing read that is not an
// argument:
//   update  moving <- moving - momentum * (moving - batch statistic)      (assign_moving_average, no zero-debias)
//   load    Layer::mean / rstd <- moving_mean, 1 / sqrt(moving_variance + eps)   (what every consumer reads in frozen mode)
// The update is evaluated in fp64 with every operation rounded on its own (no FMA contraction) and rounded to fp32 once, so
//     np.float32(m - mu * (m - x))    on float64 operands
// reproduces it bit for bit.  The batch variance comes from the stored fp32 rstd: v = max(1 / (rstd * rstd) - eps, 0).
#include <string.h>

#include "bn_moving.h"

namespace {

// Plain operators under contract(off): the instructions then carry no `contract` flag and cannot be fused.  (The __dmul_rn /
// __dsub_rn wrappers of the HIP headers are compiled under the header's own contraction mode: the backend fused their product and
// difference into one v_fma_f64, which differs from the two-rounding result in the last fp32 bit now and then.)
__device__ __forceinline__ float bnm_fold(float moving, double x, double mu) {
#pragma clang fp contract(off)
  const double m = (double)moving;
  const double d = m - x;
  const double p = mu * d;
  const double r = m - p;
  return (float)r;
}

__device__ __forceinline__ double bnm_batch_var(float rstd, double eps) {
#pragma clang fp contract(off)
  const double r = (double)rstd;
  const double rr = r * r;
  const double q = 1.0 / rr;     // the IEEE correctly rounded fp64 division (div_scale / div_fmas / div_fixup)
  const double v = q - eps;
  return v > 0.0 ? v : 0.0;
}

// table != nullptr: layer blockIdx.y of the table, its block of `moving` at e.off; else the single entry `one` with the
// moving mean at `moving` and the moving variance at `mvar` (the bare op's flat vectors)
__global__ __launch_bounds__(256) void bnm_update_kernel(const BnmEntry* __restrict__ table, BnmEntry one, float* moving, float* mvar,
                                                         double mu, double eps) {
  const BnmEntry e = table ? table[blockIdx.y] : one;
  float* mm = moving + e.off;
  float* mv = mvar ? mvar : mm + e.C;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < e.C; c += gridDim.x * 256) {
    const double x = (double)e.mean[c];
    const double v = bnm_batch_var(e.rstd[c], eps);
    mm[c] = bnm_fold(mm[c], x, mu);
    mv[c] = bnm_fold(mv[c], v, mu);
  }
}

// rstd as the kernels' own finalise forms it (bn_stats_final_kernel, elementwise.hip); pad lanes [C, stride) get 0
__global__ __launch_bounds__(256) void bnm_load_kernel(const BnmEntry* __restrict__ table, const float* __restrict__ moving, float eps) {
  const BnmEntry e = table[blockIdx.y];
  const float* mm = moving + e.off;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < e.stride; c += gridDim.x * 256) {
    float m = 0.f, r = 0.f;
    if (c < e.C) {
      m = mm[c];
      r = (float)(1.0 / sqrt((double)mm[e.C + c] + (double)eps));
    }
    e.mean[c] = m;
    e.rstd[c] = r;
  }
}

}  // namespace

void bnm_plan(BnmState& st, Arena& A) {
  st.max_stride = 0;
  st.total = 0;
  for (BnmEntry& e : st.host) {
    e.off = st.total;
    st.total += 2 * (int64_t)e.C;
    if (e.stride > st.max_stride) st.max_stride = e.stride;
  }
  st.table = (BnmEntry*)A.take(st.host.size() * sizeof(BnmEntry));
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) st.scratch[i][j] = A.floats(st.max_stride);
}

int bnm_upload(BnmState& st) {
  URSN_HIP(hipMemcpy(st.table, st.host.data(), st.host.size() * sizeof(BnmEntry), hipMemcpyHostToDevice));
  return 0;
}

int bnm_launch_load(const BnmState& st, hipStream_t s) {
  const dim3 grid((unsigned)((st.max_stride + 255) / 256), (unsigned)st.host.size());
  ursn_note_kernel("bn_frozen_load");
  hipLaunchKernelGGL(bnm_load_kernel, grid, dim3(256), 0, s, (const BnmEntry*)st.table, (const float*)st.moving, st.eps);
  URSN_HIP(hipGetLastError());
  return 0;
}

int bnm_launch_update(const BnmState& st, double momentum, hipStream_t s) {
  const dim3 grid((unsigned)((st.max_stride + 255) / 256), (unsigned)st.host.size());
  BnmEntry none;
  memset(&none, 0, sizeof(none));
  ursn_note_kernel("bn_moving_update");
  hipLaunchKernelGGL(bnm_update_kernel, grid, dim3(256), 0, s, (const BnmEntry*)st.table, none, st.moving, (float*)nullptr, momentum,
                     (double)st.eps);
  URSN_HIP(hipGetLastError());
  return 0;
}

// The bare op: the same kernel on flat contiguous vectors.  Every refusal returns before any device access.
extern "C" int ursn_bn_moving_update(const float* mean, const float* rstd, float* moving_mean, float* moving_variance, int64_t count,
                                     double momentum, float eps, void* stream) {
  URSN_REQUIRE(mean && rstd && moving_mean && moving_variance, "bn_moving_update: null mean / rstd / moving_mean / moving_variance");
  URSN_REQUIRE(count >= 1 && count < ((int64_t)1 << 31), "bn_moving_update: count = %lld outside [1, 2^31)", (long long)count);
  URSN_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "bn_moving_update: momentum = %g outside [0, 1]", momentum);
  URSN_REQUIRE(eps > 0.f, "bn_moving_update: eps = %g must be positive", (double)eps);
  URSN_REQUIRE((((uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)moving_mean | (uintptr_t)moving_variance) & 3) == 0,
               "bn_moving_update: pointers must be 4-byte aligned");
  BnmEntry one;
  memset(&one, 0, sizeof(one));
  one.mean = const_cast<float*>(mean); one.rstd = const_cast<float*>(rstd); one.C = (int32_t)count; one.stride = (int32_t)count;
  int64_t blocks = cdiv64(count, 256);
  if (blocks > 1024) blocks = 1024;
  ursn_note_kernel("bn_moving_update");
  hipLaunchKernelGGL(bnm_update_kernel, dim3((unsigned)blocks, 1), dim3(256), 0, (hipStream_t)stream, (const BnmEntry*)nullptr, one,
                     moving_mean, moving_variance, momentum, (double)eps);
  URSN_HIP(hipGetLastError());
  return 0;
}
