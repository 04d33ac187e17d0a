// Voxel-list I/O at the boundary of the dense network (gfx950): ursn_voxels_to_dense expands a batch of larcv-style voxel
// lists into the dense fp32 tensors the kernels read, ursn_labels_to_voxels compacts a dense label volume into the voxel
// set the reference writes (larcv.as_tensor3d into a sparse3d product, lib/ssnet_trainval.py:299-302), ursn_scores_at_voxels
// gathers class scores / argmax / ana label at an event's own voxels from the stored logits.  All are stateless
// op-level passes: HBM-bound streaming kernels, no atomics, no workgroup waits on another, nothing read that the same call
// did not write (the scratch buffer needs no initialisation), so the same arguments give the same bits.
#include "bf16_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Fill stores: 0 plain, 1 non-temporal.  The expanded tensors are read straight away by conv0 and by the head, so plain stores
// (which keep the lines in L2 / the Infinity Cache) are the default; DESIGN.md "Voxel-list I/O" has the A/B.
#ifndef URSN_VOXEL_FILL_NT
#define URSN_VOXEL_FILL_NT 0
#endif

// ---- ursn_voxels_to_dense ------------------------------------------------------------------------------------------------
struct VoxFillArgs {
  float* out[3];     // data, label, weight; nullptr: role not asked for
  const float* bg;   // [n] background of the weight role (data / label background is 0)
  int n;
  int64_t V;
};

// Each role is ONE flat array of n * V floats: `h` < 4 scalar elements up to the first 16-byte boundary, Q aligned float4s,
// < 4 scalar elements of tail.  blockIdx.y = event, blockIdx.z = role; an event owns the float4s whose FIRST element lies in
// it, so with V % 4 != 0 its last float4 reaches into the next event(s) and takes their background per component.
__global__ __launch_bounds__(256) void voxel_fill_kernel(VoxFillArgs a) {
  float* out = a.out[blockIdx.z];
  if (!out) return;
  const float* bg = blockIdx.z == 2 ? a.bg : nullptr;
  const int e = blockIdx.y;
  const int64_t V = a.V, total = (int64_t)a.n * V;
  int64_t h = (int64_t)(((16 - ((uintptr_t)out & 15)) & 15) >> 2);
  if (h > total) h = total;
  const int64_t Q = (total - h) >> 2;
  f32x4* A = (f32x4*)(out + h);
  const int64_t lo = (int64_t)e * V, hi = lo + V;
  const int64_t qlo = lo <= h ? 0 : (lo - h + 3) >> 2;
  int64_t qhi = hi <= h ? 0 : (hi - h + 3) >> 2;
  if (qhi > Q) qhi = Q;
  const float v = bg ? bg[e] : 0.f;
  for (int64_t q = qlo + (int64_t)blockIdx.x * 256 + threadIdx.x; q < qhi; q += (int64_t)gridDim.x * 256) {
    f32x4 x = {v, v, v, v};
    const int64_t p = h + 4 * q;
    if (bg && p + 3 >= hi) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = bg[(p + j) / V];
    }
#if URSN_VOXEL_FILL_NT
    __builtin_nontemporal_store(x, A + q);
#else
    A[q] = x;
#endif
  }
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const int64_t t = threadIdx.x;
    if (e == 0 && t < h) out[t] = bg ? bg[t / V] : 0.f;
    const int64_t p = h + 4 * Q + t;
    if (e == a.n - 1 && p < total) out[p] = bg ? bg[p / V] : 0.f;
  }
}

// One thread per list entry; blockIdx.y = event.  Indices are strictly increasing inside an event, so no two threads share
// an address; an index outside [0, V) is skipped (safety net: VoxelBatch.validate() refuses such a list on the host).
__global__ __launch_bounds__(256) void voxel_scatter_kernel(ursn_voxel_batch b, float* __restrict__ data,
                                                            float* __restrict__ label, float* __restrict__ weight) {
  const int e = blockIdx.y;
  int64_t lo = b.offsets[e];
  const int64_t hi = b.offsets[e + 1];
  if (lo < 0) lo = 0;
  const int64_t base = (int64_t)e * b.voxels;
  for (int64_t j = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; j < hi; j += (int64_t)gridDim.x * 256) {
    const int32_t i = b.index[j];
    if ((uint32_t)i >= (uint32_t)b.voxels) continue;
    data[base + i] = b.value[j];
    if (label) label[base + i] = b.label[j];
    if (weight) weight[base + i] = b.weight[j];
  }
}

static int check_dims(const char* who, int32_t n, int64_t voxels) {
  URSN_REQUIRE(n >= 1 && n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)n);
  URSN_REQUIRE(voxels >= 1, "%s: voxels = %lld < 1", who, (long long)voxels);
  URSN_REQUIRE(voxels < ((int64_t)1 << 31), "%s: voxels = %lld >= 2^31 (indices are int32)", who, (long long)voxels);
  return 0;
}

// ursn_voxels_to_dense's argument checks and its fill pass; ursn_voxels_to_dense_sym (symmetry.hip) shares them
int launch_voxel_fill(const ursn_voxel_batch* b, float* data, float* label, float* weight, hipStream_t s) {
  URSN_REQUIRE(b && data, "voxels_to_dense: null batch or data output");
  URSN_TRY(check_dims("voxels_to_dense", b->n, b->voxels));
  URSN_REQUIRE(b->offsets && b->index && b->value, "voxels_to_dense: null offsets / index / value");
  URSN_REQUIRE(!label || b->label, "voxels_to_dense: label output without a label list");
  URSN_REQUIRE((weight != nullptr) == (b->weight != nullptr), "voxels_to_dense: weight list and weight output must come together");
  URSN_REQUIRE(!weight || b->bg_weight, "voxels_to_dense: null bg_weight with a weight output");
  URSN_REQUIRE((((uintptr_t)data | (uintptr_t)label | (uintptr_t)weight) & 3) == 0, "voxels_to_dense: outputs must be 4-byte aligned");
  VoxFillArgs f;
  f.out[0] = data, f.out[1] = label, f.out[2] = weight;
  f.bg = b->bg_weight, f.n = b->n, f.V = b->voxels;
  // 4 float4 per thread and grid pass; the grid-stride loop takes the rest
  int64_t fx = cdiv64(cdiv64(b->voxels, 4), 256 * 4);
  fx = fx < 1 ? 1 : fx > 2048 ? 2048 : fx;
  ursn_note_kernel("voxel_fill");
  hipLaunchKernelGGL(voxel_fill_kernel, dim3((unsigned)fx, (unsigned)b->n, 3), dim3(256), 0, s, f);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_voxels_to_dense(const ursn_voxel_batch* b, float* data, float* label, float* weight, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  URSN_TRY(launch_voxel_fill(b, data, label, weight, s));
  // the list length lives on the device (offsets[n]): a grid sized for the usual occupancy, grid-stride for a denser event
  int64_t sx = cdiv64(b->voxels, 256 * 8);
  sx = sx < 1 ? 1 : sx > 1024 ? 1024 : sx;
  ursn_note_kernel("voxel_scatter");
  hipLaunchKernelGGL(voxel_scatter_kernel, dim3((unsigned)sx, (unsigned)b->n), dim3(256), 0, s, *b, data, label, weight);
  URSN_HIP(hipGetLastError());
  return 0;
}

// ---- ursn_labels_to_voxels -----------------------------------------------------------------------------------------------
// A workgroup owns a fixed span of VOX_SPAN consecutive voxels of one event, each of its 4 waves a contiguous quarter, a lane
// voxel (quarter start + 64 t + lane) in iteration t: ballot bit order == voxel order.
#define VOX_ITER 8
#define VOX_SPAN (256 * VOX_ITER)

static inline int64_t vox_blocks(int64_t voxels) { return cdiv64(voxels, VOX_SPAN); }

__device__ __forceinline__ int vox_wave_ballots(const float* __restrict__ L, int64_t V, int64_t v0, int lane,
                                                unsigned long long (&m)[VOX_ITER], float (&val)[VOX_ITER]) {
  int c = 0;
#pragma unroll
  for (int t = 0; t < VOX_ITER; ++t) {
    const int64_t v = v0 + t * 64 + lane;
    val[t] = v < V ? L[v] : 0.f;
    m[t] = __ballot(val[t] != 0.f);
    c += __popcll(m[t]);
  }
  return c;
}

// launch 1: counts[event][block] = non-zero labels in the block's span
__global__ __launch_bounds__(256) void voxel_count_kernel(const float* __restrict__ labels, int64_t V, int32_t* __restrict__ counts) {
  __shared__ int sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* L = labels + (int64_t)blockIdx.y * V;
  unsigned long long m[VOX_ITER];
  float val[VOX_ITER];
  const int c = vox_wave_ballots(L, V, (int64_t)blockIdx.x * VOX_SPAN + wave * (64 * VOX_ITER), lane, m, val);
  if (lane == 0) sm[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// launch 2: ONE workgroup turns the counts into exclusive prefixes inside each event (in place) and walks the events in order
// for offsets_out -- a fixed order, nobody to wait for.  A thread owns a contiguous chunk of an event's blocks.
__global__ __launch_bounds__(1024) void voxel_scan_kernel(int32_t* __restrict__ counts, int n, int64_t B,
                                                          int64_t* __restrict__ offsets_out) {
  __shared__ int wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = (B + 1023) / 1024;
  int64_t lo = threadIdx.x * chunk, hi = lo + chunk;
  if (lo > B) lo = B;
  if (hi > B) hi = B;
  int64_t running = 0;
  for (int e = 0; e < n; ++e) {
    int32_t* c = counts + (int64_t)e * B;
    int s = 0;
    for (int64_t i = lo; i < hi; ++i) s += c[i];
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    int excl = before + incl - s;
    for (int64_t i = lo; i < hi; ++i) {
      const int t = c[i];
      c[i] = excl;
      excl += t;
    }
    if (threadIdx.x == 0) offsets_out[e] = running;
    running += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets_out[n] = running;
}

// launch 3: the voxel set, at offsets[event] + prefix[block] + the LDS scan of the wave counts + the rank inside the ballot
__global__ __launch_bounds__(256) void voxel_write_kernel(const float* __restrict__ labels, int64_t V,
                                                          const int32_t* __restrict__ prefix, const int64_t* __restrict__ offsets,
                                                          int32_t* __restrict__ index_out, uint8_t* __restrict__ class_out,
                                                          int64_t cap) {
  __shared__ int sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* L = labels + (int64_t)blockIdx.y * V;
  const int64_t v0 = (int64_t)blockIdx.x * VOX_SPAN + wave * (64 * VOX_ITER);
  unsigned long long m[VOX_ITER];
  float val[VOX_ITER];
  const int c = vox_wave_ballots(L, V, v0, lane, m, val);
  if (lane == 0) sm[wave] = c;
  __syncthreads();
  int woff = 0;
  for (int w = 0; w < wave; ++w) woff += sm[w];
  int64_t pos = offsets[blockIdx.y] + prefix[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] + woff;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int t = 0; t < VOX_ITER; ++t) {
    if ((m[t] >> lane) & 1ull) {
      const int64_t p = pos + __popcll(m[t] & below);
      if (p < cap) {
        index_out[p] = (int32_t)(v0 + t * 64 + lane);
        class_out[p] = (uint8_t)(int)val[t];
      }
    }
    pos += __popcll(m[t]);
  }
}

extern "C" size_t ursn_labels_to_voxels_scratch_bytes(int32_t n, int64_t voxels) {
  if (n < 1 || voxels < 1) return 0;
  return (size_t)n * (size_t)vox_blocks(voxels) * sizeof(int32_t);
}

extern "C" int ursn_labels_to_voxels(const float* labels, int32_t n, int64_t voxels, int32_t* index_out, uint8_t* class_out,
                                     int64_t cap, int64_t* offsets_out, void* scratch, size_t scratch_bytes, void* stream) {
  URSN_REQUIRE(labels && index_out && class_out && offsets_out && scratch, "labels_to_voxels: null pointer");
  URSN_TRY(check_dims("labels_to_voxels", n, voxels));
  URSN_REQUIRE(cap >= 0, "labels_to_voxels: cap = %lld < 0", (long long)cap);
  const size_t need = ursn_labels_to_voxels_scratch_bytes(n, voxels);
  URSN_REQUIRE(scratch_bytes >= need, "labels_to_voxels: scratch of %zu bytes is too small, %zu needed", scratch_bytes, need);
  URSN_REQUIRE(((uintptr_t)scratch & 3) == 0 && ((uintptr_t)offsets_out & 7) == 0 && ((uintptr_t)index_out & 3) == 0,
               "labels_to_voxels: scratch / index_out must be 4-byte, offsets_out 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = vox_blocks(voxels);
  int32_t* counts = (int32_t*)scratch;
  const dim3 grid((unsigned)B, (unsigned)n);
  ursn_note_kernel("voxel_count");
  hipLaunchKernelGGL(voxel_count_kernel, grid, dim3(256), 0, s, labels, voxels, counts);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("voxel_scan");
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(1024), 0, s, counts, (int)n, B, offsets_out);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("voxel_write");
  hipLaunchKernelGGL(voxel_write_kernel, grid, dim3(256), 0, s, labels, voxels, (const int32_t*)counts,
                     (const int64_t*)offsets_out, index_out, class_out, cap);
  URSN_HIP(hipGetLastError());
  return 0;
}

// ---- ursn_scores_at_voxels -----------------------------------------------------------------------------------------------
// The gather head: one thread per list entry, blockIdx.y = event (its entries are [offsets[e], offsets[e + 1])), grid-stride
// inside the event.  The arithmetic RESTATES the dense heads' (head_kernel in elementwise.hip, bhead_kernel in
// bf16_elementwise.hip) statement by statement -- fmaf(raw, sc, sh) with sh = beta - mean * sc, strict '>' argmax, exp(z - m)
// summed in class order, e * (1 / sum), the ana rule on the products -- so the scores are the bits the dense softmax holds at
// the same voxel; tests/test_voxel_scores_gpu.py compares them bit for bit on both plans.  (Restated, not shared through a
// __device__ helper: the heads are the benchmark's kernels and their generated code stays untouched.)  DT: 0 fp32 logits and
// expf (fp32 head), 1 bf16 logits and __expf (bf16 head).  V4: <= 4 classes in 4-padded, 16-byte aligned fp32 logits, one
// 16-byte load.
struct VScoreArgs {
  ursn_vscores_desc d;
  float* scores;
  uint8_t* pred;
  uint8_t* ana;
  int64_t cap;   // rows at or beyond cap are never written (the caller's buffers hold cap rows)
};

template <int DT, bool V4>
__global__ __launch_bounds__(256) void vscores_kernel(VScoreArgs a) {
  const ursn_vscores_desc& d = a.d;
  const int e = blockIdx.y;
  int64_t lo = d.offsets[e], hi = d.offsets[e + 1];
  if (lo < 0) lo = 0;
  if (hi > a.cap) hi = a.cap;
  const int ncls = d.ncls;
  float sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sc[k] = 1.f;
    sh[k] = 0.f;
    if (k < ncls && d.mean) {
      sc[k] = d.rstd[k];
      sh[k] = d.beta[k] - d.mean[k] * sc[k];
    }
  }
  const int64_t base = (int64_t)e * d.voxels;
  for (int64_t j = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; j < hi; j += (int64_t)gridDim.x * 256) {
    const int32_t i = d.index[j];
    float pr[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) pr[k] = 0.f;
    int arg = 0, lab = 0;
    if ((uint32_t)i < (uint32_t)d.voxels) {   // an index outside [0, voxels) reads nothing: its rows are zeros
      const int64_t p = base + i;
      float raw[8];
      if constexpr (DT == 1) {
        unpack8(*(const u32x4*)((const bf16_t*)d.z + p * 8), raw);
      } else if constexpr (V4) {
        const f32x4 zv = *(const f32x4*)((const float*)d.z + p * 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) raw[k] = k < 4 ? zv[k & 3] : 0.f;
      } else {
        const float* zp = (const float*)d.z + p * d.z_cstride;
#pragma unroll
        for (int k = 0; k < 8; ++k) raw[k] = k < ncls ? zp[k] : 0.f;
      }
      float z[8], ex[8];
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) {
          z[k] = fmaf(raw[k], sc[k], sh[k]);
          if (z[k] > m) { m = z[k]; arg = k; }   // strict '>' keeps the lowest index on ties
        }
      float ssum = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) {
          if constexpr (DT == 1) ex[k] = __expf(z[k] - m);
          else ex[k] = expf(z[k] - m);
          ssum += ex[k];
        }
      const float inv = 1.0f / ssum;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) pr[k] = ex[k] * inv;
      if (a.ana) {   // (shower > track) * 1 + (track >= shower) * 2, masked by data > 1.0 (lib/ssnet_trainval.py:285-287)
        const float shower = ex[1] * inv, track = ex[2] * inv;
        const int rule = (shower > track ? 1 : 0) + (track >= shower ? 2 : 0);
        lab = d.data[p] > 1.0f ? rule : 0;
      }
    }
    if (a.scores) {
      float* o = a.scores + j * ncls;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) o[k] = pr[k];
    }
    if (a.pred) a.pred[j] = (uint8_t)arg;
    if (a.ana) a.ana[j] = (uint8_t)lab;
  }
}

// m_total < 0: the list length is not known on the host (op level): grid sized from `voxels`, every row an entry names may be
// written.  m_total >= 0 (net level): no event holds more than m_total entries, rows >= m_total are never written, 0 launches nothing.
int launch_vscores(const ursn_vscores_desc* d, float* scores_out, uint8_t* pred_out, uint8_t* ana_out, int64_t m_total,
                   hipStream_t s) {
  URSN_REQUIRE(d && d->offsets && d->index && d->z, "scores_at_voxels: null desc / offsets / index / z");
  URSN_REQUIRE(scores_out || pred_out || ana_out, "scores_at_voxels: all three outputs are null");
  URSN_TRY(check_dims("scores_at_voxels", d->n, d->voxels));
  URSN_REQUIRE(d->ncls >= 1 && d->ncls <= 8, "scores_at_voxels: num_class %d not in [1,8]", (int)d->ncls);
  URSN_REQUIRE(!ana_out || d->ncls >= 3, "scores_at_voxels: ana_out needs >= 3 classes (num_class = %d)", (int)d->ncls);
  URSN_REQUIRE(!ana_out || d->data, "scores_at_voxels: ana_out needs data (the data > 1.0 mask)");
  URSN_REQUIRE(d->dtype == 0 || d->dtype == 1, "scores_at_voxels: dtype %d not in {0 fp32, 1 bf16}", (int)d->dtype);
  if (d->dtype == 1) {
    URSN_REQUIRE(d->z_cstride == 8, "scores_at_voxels: bf16 logits need channel stride 8 (z_cstride = %d)", (int)d->z_cstride);
    URSN_REQUIRE(((uintptr_t)d->z & 15) == 0, "scores_at_voxels: bf16 logits must be 16-byte aligned");
  } else {
    URSN_REQUIRE(d->z_cstride >= d->ncls, "scores_at_voxels: z_cstride %d < num_class %d", (int)d->z_cstride, (int)d->ncls);
    URSN_REQUIRE(((uintptr_t)d->z & 3) == 0, "scores_at_voxels: fp32 logits must be 4-byte aligned");
  }
  URSN_REQUIRE(!d->mean || (d->rstd && d->beta), "scores_at_voxels: mean without rstd / beta");
  URSN_REQUIRE(((uintptr_t)scores_out & 3) == 0 && ((uintptr_t)d->offsets & 7) == 0 && ((uintptr_t)d->index & 3) == 0,
               "scores_at_voxels: scores_out / index must be 4-byte, offsets 8-byte aligned");
  if (m_total == 0) return 0;
  VScoreArgs a;
  a.d = *d;
  a.scores = scores_out, a.pred = pred_out, a.ana = ana_out;
  a.cap = m_total < 0 ? INT64_MAX : m_total;
  int64_t gx = m_total < 0 ? cdiv64(d->voxels, 256 * 8) : cdiv64(m_total, 256);
  gx = gx < 1 ? 1 : gx > 1024 ? 1024 : gx;
  const dim3 grid((unsigned)gx, (unsigned)d->n);
  ursn_note_kernel("vscores");
  if (d->dtype == 1) hipLaunchKernelGGL((vscores_kernel<1, false>), grid, dim3(256), 0, s, a);
  else if (d->z_cstride == 4 && d->ncls <= 4 && ((uintptr_t)d->z & 15) == 0) hipLaunchKernelGGL((vscores_kernel<0, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((vscores_kernel<0, false>), grid, dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_scores_at_voxels(const ursn_vscores_desc* d, float* scores_out, uint8_t* pred_out, uint8_t* ana_out,
                                     void* stream) {
  return launch_vscores(d, scores_out, pred_out, ana_out, -1, (hipStream_t)stream);
}
