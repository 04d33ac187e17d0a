// Per-event normalisation of the loss weights (gfx950): ursn_normalize_weights divides every event's pixel weights by the
// event's sum, what the reference does on the host before it feeds a minibatch (lib/ssnet_trainval.py:173,204).  A stateless
// op-level pass like those of voxel_io.hip: two HBM-bound streaming launches, no atomics, no workgroup waits on another,
// nothing read that the same call did not write (the scratch buffer needs no initialisation), so the same arguments give the
// same bits.
#include "ursn_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// A workgroup owns a fixed span of WNORM_SPAN consecutive voxels of one event (blockIdx.x = span, blockIdx.y = event): the
// span is a compile-time constant, so which values meet in which partial sum never depends on the launch geometry.  Inside a
// span: `h` < 4 scalar elements up to the first 16-byte boundary, Q <= 256 * WNORM_ITER aligned float4s (thread t owns float4
// t + 256 i), < 4 scalar elements of tail.  An event starts e * voxels floats into the tensor, so the split is taken from the
// ADDRESS of the span (voxels % 4 != 0, or a tensor that is only 4-byte aligned, moves it); the span length is a multiple of 16
// bytes, so all full spans of one event split alike.
#define WNORM_ITER 16
#define WNORM_SPAN (256 * 4 * WNORM_ITER)

static inline int64_t wnorm_blocks(int64_t voxels) { return cdiv64(voxels, WNORM_SPAN); }

struct WnormSpan {
  int len, h, Q, tail;
};

__device__ __forceinline__ WnormSpan wnorm_span(const float* p, int64_t V, int64_t lo) {
  WnormSpan s;
  const int64_t left = V - lo;
  s.len = left < WNORM_SPAN ? (int)left : WNORM_SPAN;
  s.h = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  if (s.h > s.len) s.h = s.len;
  s.Q = (s.len - s.h) >> 2;
  s.tail = s.len - s.h - 4 * s.Q;
  return s;
}

// Sum of one double per thread over the workgroup, the same value in every thread: lanes by shuffles in a fixed order, then
// the four waves through LDS in wave order.
__device__ __forceinline__ double wnorm_block_sum(double acc, double* sm) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// launch 1: partial[event][span] = fp64 sum of the span; writes nothing else
__global__ __launch_bounds__(256) void wnorm_sum_kernel(const float* __restrict__ w, int64_t V, double* __restrict__ partial) {
  __shared__ double sm[4];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * WNORM_SPAN;
  const float* p = w + (int64_t)blockIdx.y * V + lo;
  const WnormSpan s = wnorm_span(p, V, lo);
  const f32x4* A = (const f32x4*)(p + s.h);
  f32x4 x[WNORM_ITER];
#pragma unroll
  for (int i = 0; i < WNORM_ITER; ++i)
    if (t + 256 * i < s.Q) x[i] = A[t + 256 * i];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int i = 0; i < WNORM_ITER; ++i)
    if (t + 256 * i < s.Q) {
      a0 += (double)x[i][0];
      a1 += (double)x[i][1];
      a2 += (double)x[i][2];
      a3 += (double)x[i][3];
    }
  double acc = (a0 + a1) + (a2 + a3);
  if (t < s.h) acc += (double)p[t];
  if (t < s.tail) acc += (double)p[s.h + 4 * s.Q + t];
  acc = wnorm_block_sum(acc, sm);
  if (t == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// launch 2: every workgroup reduces its event's partials by the same fixed tree (thread t takes partials t, t + 256, ... in
// order, then wnorm_block_sum), so all of them hold the same S_e; rounded once to fp32; out = w / (float)S_e over the span with
// the correctly rounded division.  `out` may be `w` itself: a thread reads what it overwrites before it writes.  The 16-byte
// path needs w and out equally placed inside their 16-byte lines; a differently aligned pair goes element by element.
__global__ __launch_bounds__(256) void wnorm_scale_kernel(const float* w, float* out, int64_t V, const double* __restrict__ partial,
                                                          float* __restrict__ sums_out) {
  __shared__ double sm[4];
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * WNORM_SPAN;
  const int64_t at = (int64_t)blockIdx.y * V + lo;
  const float* p = w + at;
  float* o = out + at;
  const WnormSpan s = wnorm_span(p, V, lo);
  const bool vec = (((uintptr_t)p ^ (uintptr_t)o) & 15) == 0;
  const f32x4* A = (const f32x4*)(p + s.h);
  f32x4 x[WNORM_ITER];
  if (vec) {   // the span's loads are in flight while the partials are reduced
#pragma unroll
    for (int i = 0; i < WNORM_ITER; ++i)
      if (t + 256 * i < s.Q) x[i] = A[t + 256 * i];
  }
  const double* P = partial + (int64_t)blockIdx.y * gridDim.x;
  double acc = 0.0;
  for (int i = t; i < (int)gridDim.x; i += 256) acc += P[i];
  const float S = (float)wnorm_block_sum(acc, sm);
  if (blockIdx.x == 0 && t == 0 && sums_out) sums_out[blockIdx.y] = S;
  if (vec) {
    f32x4* O = (f32x4*)(o + s.h);
#pragma unroll
    for (int i = 0; i < WNORM_ITER; ++i)
      if (t + 256 * i < s.Q) {
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = __fdiv_rn(x[i][j], S);
        O[t + 256 * i] = y;
      }
    if (t < s.h) o[t] = __fdiv_rn(p[t], S);
    if (t < s.tail) o[s.h + 4 * s.Q + t] = __fdiv_rn(p[s.h + 4 * s.Q + t], S);
  } else {
    for (int i = t; i < s.len; i += 256) o[i] = __fdiv_rn(p[i], S);
  }
}

static inline bool wnorm_dims_ok(int32_t n, int64_t voxels) {
  return n >= 1 && n <= 65535 && voxels >= 1 && voxels < ((int64_t)1 << 31);
}

extern "C" size_t ursn_normalize_weights_scratch_bytes(int32_t n, int64_t voxels) {
  if (!wnorm_dims_ok(n, voxels)) return 0;
  return (size_t)n * (size_t)wnorm_blocks(voxels) * sizeof(double);
}

extern "C" int ursn_normalize_weights(const float* weight, float* out, int32_t n, int64_t voxels, float* sums_out, void* scratch,
                                      size_t scratch_bytes, void* stream) {
  URSN_REQUIRE(weight && out && scratch, "normalize_weights: null weight / out / scratch");
  URSN_REQUIRE(n >= 1 && n <= 65535, "normalize_weights: n = %d outside [1, 65535]", (int)n);
  URSN_REQUIRE(voxels >= 1, "normalize_weights: voxels = %lld < 1", (long long)voxels);
  URSN_REQUIRE(voxels < ((int64_t)1 << 31), "normalize_weights: voxels = %lld >= 2^31", (long long)voxels);
  const size_t need = ursn_normalize_weights_scratch_bytes(n, voxels);
  URSN_REQUIRE(scratch_bytes >= need, "normalize_weights: scratch of %zu bytes is too small, %zu needed", scratch_bytes, need);
  URSN_REQUIRE(((uintptr_t)scratch & 7) == 0, "normalize_weights: scratch must be 8-byte aligned");
  URSN_REQUIRE((((uintptr_t)weight | (uintptr_t)out | (uintptr_t)sums_out) & 3) == 0,
               "normalize_weights: weight / out / sums_out must be 4-byte aligned");
  const uintptr_t wa = (uintptr_t)weight, oa = (uintptr_t)out, bytes = (uintptr_t)n * (uintptr_t)voxels * sizeof(float);
  URSN_REQUIRE(wa == oa || wa + bytes <= oa || oa + bytes <= wa,
               "normalize_weights: out overlaps weight without being equal to it (in place needs out == weight)");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)wnorm_blocks(voxels), (unsigned)n);
  double* partial = (double*)scratch;
  ursn_note_kernel("wnorm_sum");
  hipLaunchKernelGGL(wnorm_sum_kernel, grid, dim3(256), 0, s, weight, voxels, partial);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("wnorm_scale");
  hipLaunchKernelGGL(wnorm_scale_kernel, grid, dim3(256), 0, s, weight, out, voxels, (const double*)partial, sums_out);
  URSN_HIP(hipGetLastError());
  return 0;
}
