// Tiling at the voxel-list boundary (gfx950): ursn_crop_count / ursn_crop_write cut boxes of one tile size out of large events
// given as voxel lists and hand each box over as an event of a complete ursn_voxel_batch at the tile's size (what
// ursn_voxels_to_dense, ursn_voxels_to_dense_sym and ursn_infer_voxels take), ursn_scores_scatter copies the gather head's rows of
// the voxels a box OWNS back to the large event's own list order.  Stateless op-level passes like voxel_io.hip's: no atomics, no
// workgroup waits on another, nothing read that the same call did not write (the scratch needs no initialisation), so the same
// arguments give the same bits.
//
// A large event's list is sorted row-major, so the entries whose slowest coordinate lies in a box's extent along that axis are ONE
// contiguous range of the list: crop_range_kernel finds it with two binary searches per box.  Subtracting the origin keeps the
// order, so a STABLE compaction of the range by "inside the box" is already the box's sorted list -- nothing is sorted and a box
// never reads the rest of the list.  The range is cut into P = 4 G contiguous parts (G workgroups of 4 waves per box, G fixed by the
// shapes alone), a wave walks its part 64 entries at a time and ranks the survivors with ballot / popcount: ballot bit order ==
// list order.  Pass 1 counts per part, one workgroup turns the counts into exclusive prefixes and box offsets in a fixed order,
// pass 2 repeats the walk and writes.
#include "ursn_common.h"

#define CROP_WAVES 4                 // waves per workgroup, each owns one part of the box's range
#define CROP_VOX_PER_GROUP 4096      // voxels of the box's slowest-axis slab per workgroup: G = ceil(slab / this), 1..CROP_MAX_GROUPS
#define CROP_MAX_GROUPS 32
#define CROP_MAX_BOXES (1 << 20)

struct CropArgs {
  ursn_crop_desc d;
  int S[3], T[3];     // the shapes as three axes (2-D: a last axis of extent 1)
  int G;              // workgroups per box
  int32_t* range;     // [B][2]  the box's range [r0, r1) of list positions
  int32_t* cnt;       // [B][P]  entries inside the box per part; after the scan: exclusive prefixes inside the box
  int32_t* own;       // [B][P]  of those, entries inside the core
  int32_t* tot;       // [B]     entries inside the box (the scan keeps them while cnt turns into prefixes)
};

static int crop_groups(const int* S, const int* T) {
  const int64_t slab = (int64_t)(T[0] < S[0] ? T[0] : S[0]) * S[1] * S[2];
  const int64_t g = cdiv64(slab, CROP_VOX_PER_GROUP);
  return (int)(g < 1 ? 1 : g > CROP_MAX_GROUPS ? CROP_MAX_GROUPS : g);
}

// first position in [lo, hi) whose index is >= key (hi if none)
__device__ __forceinline__ int64_t crop_lower_bound(const int32_t* __restrict__ index, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)index[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One thread per box.  A box of an event outside [0, n), or with no overlap with the volume along some axis, gets an empty range.
__global__ __launch_bounds__(256) void crop_range_kernel(CropArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.d.boxes) return;
  const int nd = a.d.ndim;
  const int e = a.d.box_event[b];
  int64_t r0 = 0, r1 = 0;
  if ((uint32_t)e < (uint32_t)a.d.n) {
    int64_t lo = a.d.offsets[e], hi = a.d.offsets[e + 1];
    if (lo < 0) lo = 0;
    if (hi > a.d.m_total) hi = a.d.m_total;   // rows at or beyond m_total are never read
    bool some = hi > lo;
    int64_t x_lo = 0, x_hi = 0;
    for (int ax = 0; ax < nd; ++ax) {
      const int64_t o = a.d.box_origin[b * nd + ax];
      const int64_t l = o > 0 ? o : 0, h = o + a.T[ax] < a.S[ax] ? o + a.T[ax] : a.S[ax];
      if (l >= h) some = false;
      if (ax == 0) x_lo = l, x_hi = h;
    }
    if (some) {
      const int64_t plane = (int64_t)a.S[1] * a.S[2];
      r0 = crop_lower_bound(a.d.index, lo, hi, x_lo * plane);
      r1 = crop_lower_bound(a.d.index, r0, hi, x_hi * plane);
    }
  }
  a.range[2 * b] = (int32_t)r0;
  a.range[2 * b + 1] = (int32_t)r1;
}

struct CropOutArgs {
  ursn_crop_out o;
  const int64_t* box_offsets;   // == o.offsets, read after the scan
};

// blockIdx.x = box * G + group; wave w of the workgroup owns part p = group * 4 + w of the box's range.
template <bool WRITE>
__global__ __launch_bounds__(256) void crop_pass_kernel(CropArgs a, CropOutArgs w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x / a.G;
  const int P = a.G * CROP_WAVES, p = (int)(blockIdx.x % a.G) * CROP_WAVES + wave;
  const int nd = a.d.ndim;
  const int64_t r0 = a.range[2 * b], len = (int64_t)a.range[2 * b + 1] - r0;
  const int64_t part = ((len + P - 1) / P + 63) & ~(int64_t)63;
  int64_t s = (int64_t)p * part, e = s + part;
  if (s > len) s = len;
  if (e > len) e = len;
  s += r0, e += r0;
  int64_t o[3] = {0, 0, 0}, clo[3] = {0, 0, 0}, chi[3] = {a.T[0], a.T[1], a.T[2]};
  for (int ax = 0; ax < nd; ++ax) {
    o[ax] = a.d.box_origin[b * nd + ax];
    if (a.d.core_lo) clo[ax] = a.d.core_lo[b * nd + ax], chi[ax] = a.d.core_hi[b * nd + ax];
  }
  const uint32_t S2 = (uint32_t)a.S[2], plane = (uint32_t)a.S[1] * S2;
  const uint32_t bigvox = (uint32_t)a.S[0] * plane;
  const unsigned long long below = (1ull << lane) - 1ull;
  int64_t pos = 0;
  if (WRITE) {
    pos = w.box_offsets[b] + a.cnt[b * P + p];
    if (p == 0 && lane == 0 && w.o.bg_weight) {
      const int ev = a.d.box_event[b];
      w.o.bg_weight[b] = (uint32_t)ev < (uint32_t)a.d.n ? a.d.bg_weight[ev] : 0.f;
    }
  }
  int c_in = 0, c_own = 0;
  for (int64_t j0 = s; j0 < e; j0 += 64) {
    const int64_t j = j0 + lane;
    bool in = false, owned = false;
    int32_t local = 0;
    if (j < e) {
      const uint32_t i = (uint32_t)a.d.index[j];
      if (i < bigvox) {   // an index outside the large volume belongs to no box
        const uint32_t x0 = i / plane, rem = i - x0 * plane, x1 = rem / S2, x2 = rem - x1 * S2;
        const int64_t l0 = (int64_t)x0 - o[0], l1 = (int64_t)x1 - o[1], l2 = (int64_t)x2 - o[2];
        in = l0 >= 0 && l0 < a.T[0] && l1 >= 0 && l1 < a.T[1] && l2 >= 0 && l2 < a.T[2];
        owned = in && l0 >= clo[0] && l0 < chi[0] && l1 >= clo[1] && l1 < chi[1] && l2 >= clo[2] && l2 < chi[2];
        local = (int32_t)((l0 * a.T[1] + l1) * a.T[2] + l2);
      }
    }
    const unsigned long long m = __ballot(in);
    if (WRITE) {
      if (in) {
        const int64_t q = pos + __popcll(m & below);
        if (q < w.o.cap) {
          w.o.index[q] = local;
          if (w.o.value) w.o.value[q] = a.d.value[j];
          if (w.o.label) w.o.label[q] = a.d.label[j];
          if (w.o.weight) w.o.weight[q] = a.d.weight[j];
          if (w.o.src) w.o.src[q] = (int32_t)j;
          if (w.o.owned) w.o.owned[q] = owned ? 1 : 0;
        }
      }
      pos += __popcll(m);
    } else {
      c_in += __popcll(m);
      c_own += __popcll(__ballot(owned));
    }
  }
  if (!WRITE && lane == 0) {
    a.cnt[b * P + p] = c_in;
    a.own[b * P + p] = c_own;
  }
}

// ursn_crop_count's second launch: one thread per box adds its parts in part order.
__global__ __launch_bounds__(256) void crop_sum_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ own, int64_t B,
                                                       int P, int64_t* __restrict__ count_out, int64_t* __restrict__ owned_out) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int64_t c = 0, o = 0;
  for (int p = 0; p < P; ++p) c += cnt[b * P + p], o += own[b * P + p];
  count_out[b] = c;
  owned_out[b] = o;
}

// ursn_crop_write's scan: ONE workgroup, a thread owns a contiguous chunk of boxes.  A box's part counts become exclusive prefixes in
// place and its total goes to tot; the totals are scanned over the boxes in box order (a thread's chunk serially, lanes by
// shuffles, waves through LDS in wave order) for offsets_out -- a fixed order, nobody to wait for.
__global__ __launch_bounds__(1024) void crop_scan_kernel(int32_t* __restrict__ cnt, int32_t* __restrict__ tot, int64_t B, int P,
                                                         int64_t* __restrict__ offsets_out) {
  __shared__ long long wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = (B + 1023) / 1024;
  int64_t lo = threadIdx.x * chunk, hi = lo + chunk;
  if (lo > B) lo = B;
  if (hi > B) hi = B;
  long long s = 0;
  for (int64_t b = lo; b < hi; ++b) {
    int32_t run = 0;
    for (int p = 0; p < P; ++p) {
      const int32_t t = cnt[b * P + p];
      cnt[b * P + p] = run;
      run += t;
    }
    tot[b] = run;
    s += run;
  }
  long long incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  long long before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k < wave) before += wsum[k];
    total += wsum[k];
  }
  long long excl = before + incl - s;
  for (int64_t b = lo; b < hi; ++b) {
    offsets_out[b] = excl;
    excl += tot[b];   // written by this thread above
  }
  if (threadIdx.x == 0) offsets_out[B] = total;
}

// ---- host side of the crop passes ----------------------------------------------------------------------------------------------
static int crop_shapes_ok(int32_t ndim, const int32_t* big, const int32_t* tile) {
  if ((ndim != 2 && ndim != 3) || !big || !tile) return 0;
  int64_t vb = 1, vt = 1;
  for (int i = 0; i < ndim; ++i) {
    if (big[i] < 1 || tile[i] < 1) return 0;
    vb *= big[i], vt *= tile[i];
    if (vb >= ((int64_t)1 << 31) || vt >= ((int64_t)1 << 31)) return 0;
  }
  return 1;
}

extern "C" size_t ursn_crop_scratch_bytes(int32_t ndim, const int32_t* big, const int32_t* tile, int32_t boxes) {
  if (!crop_shapes_ok(ndim, big, tile) || boxes < 1 || boxes > CROP_MAX_BOXES) return 0;
  int S[3] = {big[0], big[1], ndim == 3 ? big[2] : 1}, T[3] = {tile[0], tile[1], ndim == 3 ? tile[2] : 1};
  const size_t P = (size_t)crop_groups(S, T) * CROP_WAVES;
  return (size_t)boxes * (3 + 2 * P) * sizeof(int32_t);
}

static int crop_prepare(const char* who, const ursn_crop_desc* d, void* scratch, size_t scratch_bytes, CropArgs* a) {
  URSN_REQUIRE(d, "%s: null desc", who);
  URSN_REQUIRE(d->ndim == 2 || d->ndim == 3, "%s: ndim = %d, must be 2 or 3", who, (int)d->ndim);
  int64_t vb = 1, vt = 1;
  for (int i = 0; i < d->ndim; ++i) {
    URSN_REQUIRE(d->big[i] >= 1, "%s: big[%d] = %d < 1", who, i, (int)d->big[i]);
    URSN_REQUIRE(d->tile[i] >= 1, "%s: tile[%d] = %d < 1", who, i, (int)d->tile[i]);
    vb *= d->big[i], vt *= d->tile[i];
    URSN_REQUIRE(vb < ((int64_t)1 << 31), "%s: prod(big) >= 2^31 (indices are int32)", who);
    URSN_REQUIRE(vt < ((int64_t)1 << 31), "%s: prod(tile) >= 2^31 (indices are int32)", who);
  }
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)d->n);
  URSN_REQUIRE(d->boxes >= 1 && d->boxes <= CROP_MAX_BOXES, "%s: boxes = %d outside [1, %d]", who, (int)d->boxes, CROP_MAX_BOXES);
  URSN_REQUIRE(d->m_total >= 0 && d->m_total < ((int64_t)1 << 31), "%s: m_total = %lld outside [0, 2^31)", who,
               (long long)d->m_total);
  URSN_REQUIRE(d->offsets && d->index, "%s: null offsets / index", who);
  URSN_REQUIRE(d->box_event && d->box_origin, "%s: null box_event / box_origin", who);
  URSN_REQUIRE((d->core_lo != nullptr) == (d->core_hi != nullptr), "%s: core_lo and core_hi must come together", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE(((uintptr_t)d->offsets & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "%s: offsets / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->value | (uintptr_t)d->label | (uintptr_t)d->weight | (uintptr_t)d->bg_weight |
                 (uintptr_t)d->box_event | (uintptr_t)d->box_origin | (uintptr_t)d->core_lo | (uintptr_t)d->core_hi) & 3) == 0,
               "%s: index / value / label / weight / bg_weight / box arrays must be 4-byte aligned", who);
  const size_t need = ursn_crop_scratch_bytes(d->ndim, d->big, d->tile, d->boxes);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);
  a->d = *d;
  for (int i = 0; i < 3; ++i) a->S[i] = i < d->ndim ? d->big[i] : 1, a->T[i] = i < d->ndim ? d->tile[i] : 1;
  a->G = crop_groups(a->S, a->T);
  const int64_t B = d->boxes, P = (int64_t)a->G * CROP_WAVES;
  a->range = (int32_t*)scratch;
  a->tot = a->range + 2 * B;
  a->cnt = a->tot + B;
  a->own = a->cnt + B * P;
  return 0;
}

// the two launches both entry points start with: ranges, then the per-part counts
static int crop_launch_counts(const CropArgs& a, hipStream_t s) {
  const int64_t B = a.d.boxes;
  ursn_note_kernel("crop_range");
  hipLaunchKernelGGL(crop_range_kernel, dim3((unsigned)cdiv64(B, 256)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  CropOutArgs none = {};
  ursn_note_kernel("crop_count");
  hipLaunchKernelGGL((crop_pass_kernel<false>), dim3((unsigned)(B * a.G)), dim3(256), 0, s, a, none);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_crop_count(const ursn_crop_desc* d, int64_t* count_out, int64_t* owned_out, void* scratch, size_t scratch_bytes,
                               void* stream) {
  CropArgs a;
  URSN_TRY(crop_prepare("crop_count", d, scratch, scratch_bytes, &a));
  URSN_REQUIRE(count_out && owned_out, "crop_count: null count_out / owned_out");
  URSN_REQUIRE((((uintptr_t)count_out | (uintptr_t)owned_out) & 7) == 0, "crop_count: count_out / owned_out must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  URSN_TRY(crop_launch_counts(a, s));
  ursn_note_kernel("crop_sum");
  hipLaunchKernelGGL(crop_sum_kernel, dim3((unsigned)cdiv64(d->boxes, 256)), dim3(256), 0, s, (const int32_t*)a.cnt,
                     (const int32_t*)a.own, (int64_t)d->boxes, a.G * CROP_WAVES, count_out, owned_out);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_crop_write(const ursn_crop_desc* d, const ursn_crop_out* out, void* scratch, size_t scratch_bytes, void* stream) {
  CropArgs a;
  URSN_TRY(crop_prepare("crop_write", d, scratch, scratch_bytes, &a));
  URSN_REQUIRE(out && out->offsets && out->index, "crop_write: null out / out->offsets / out->index");
  URSN_REQUIRE(out->cap >= 0, "crop_write: cap = %lld < 0", (long long)out->cap);
  URSN_REQUIRE(!out->value || d->value, "crop_write: value output without a value list");
  URSN_REQUIRE(!out->label || d->label, "crop_write: label output without a label list");
  URSN_REQUIRE(!out->weight || d->weight, "crop_write: weight output without a weight list");
  URSN_REQUIRE((out->weight != nullptr) == (out->bg_weight != nullptr), "crop_write: weight and bg_weight outputs must come together");
  URSN_REQUIRE(!out->bg_weight || d->bg_weight, "crop_write: bg_weight output without a bg_weight array");
  URSN_REQUIRE(((uintptr_t)out->offsets & 7) == 0, "crop_write: out->offsets must be 8-byte aligned");
  URSN_REQUIRE((((uintptr_t)out->index | (uintptr_t)out->value | (uintptr_t)out->label | (uintptr_t)out->weight |
                 (uintptr_t)out->bg_weight | (uintptr_t)out->src) & 3) == 0,
               "crop_write: out->index / value / label / weight / bg_weight / src must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  URSN_TRY(crop_launch_counts(a, s));
  ursn_note_kernel("crop_scan");
  hipLaunchKernelGGL(crop_scan_kernel, dim3(1), dim3(1024), 0, s, a.cnt, a.tot, (int64_t)d->boxes, a.G * CROP_WAVES, out->offsets);
  URSN_HIP(hipGetLastError());
  CropOutArgs w;
  w.o = *out;
  w.box_offsets = out->offsets;
  ursn_note_kernel("crop_write");
  hipLaunchKernelGGL((crop_pass_kernel<true>), dim3((unsigned)((int64_t)d->boxes * a.G)), dim3(256), 0, s, a, w);
  URSN_HIP(hipGetLastError());
  return 0;
}

// ---- ursn_scores_scatter -----------------------------------------------------------------------------------------------------------
// One thread per row of the crop batch; a row that is not owned, or whose source position lies outside [0, rows_out), writes nothing.
struct ScatterArgs {
  const int32_t* src;
  const uint8_t* owned;
  int64_t m, rows_out;
  int ncls;
  const float* scores;
  const uint8_t *pred, *ana;
  float* scores_out;
  uint8_t *pred_out, *ana_out;
};

__global__ __launch_bounds__(256) void scores_scatter_kernel(ScatterArgs a) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.m; j += (int64_t)gridDim.x * 256) {
    if (!a.owned[j]) continue;
    const int64_t r = a.src[j];
    if (r < 0 || r >= a.rows_out) continue;
    if (a.scores_out) {
      const float* in = a.scores + j * a.ncls;
      float* o = a.scores_out + r * a.ncls;
      for (int k = 0; k < a.ncls; ++k) o[k] = in[k];
    }
    if (a.pred_out) a.pred_out[r] = a.pred[j];
    if (a.ana_out) a.ana_out[r] = a.ana[j];
  }
}

extern "C" int ursn_scores_scatter(const int32_t* src, const uint8_t* owned, int64_t m, int32_t ncls, const float* scores,
                                   const uint8_t* pred, const uint8_t* ana, float* scores_out, uint8_t* pred_out, uint8_t* ana_out,
                                   int64_t rows_out, void* stream) {
  URSN_REQUIRE(src && owned, "scores_scatter: null src / owned");
  URSN_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "scores_scatter: m = %lld outside [0, 2^31)", (long long)m);
  URSN_REQUIRE(rows_out >= 0 && rows_out < ((int64_t)1 << 31), "scores_scatter: rows_out = %lld outside [0, 2^31)", (long long)rows_out);
  URSN_REQUIRE(ncls >= 1 && ncls <= 8, "scores_scatter: num_class %d not in [1,8]", (int)ncls);
  URSN_REQUIRE(scores_out || pred_out || ana_out, "scores_scatter: all three outputs are null");
  URSN_REQUIRE((scores != nullptr) == (scores_out != nullptr), "scores_scatter: scores and scores_out must come together");
  URSN_REQUIRE((pred != nullptr) == (pred_out != nullptr), "scores_scatter: pred and pred_out must come together");
  URSN_REQUIRE((ana != nullptr) == (ana_out != nullptr), "scores_scatter: ana and ana_out must come together");
  URSN_REQUIRE((((uintptr_t)src | (uintptr_t)scores | (uintptr_t)scores_out) & 3) == 0,
               "scores_scatter: src / scores / scores_out must be 4-byte aligned");
  if (m == 0 || rows_out == 0) return 0;
  ScatterArgs a;
  a.src = src, a.owned = owned, a.m = m, a.rows_out = rows_out, a.ncls = ncls;
  a.scores = scores, a.pred = pred, a.ana = ana;
  a.scores_out = scores_out, a.pred_out = pred_out, a.ana_out = ana_out;
  int64_t gx = cdiv64(m, 256);
  gx = gx > 4096 ? 4096 : gx;
  ursn_note_kernel("scores_scatter");
  hipLaunchKernelGGL(scores_scatter_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
