// Per-cluster charge profiles along the principal axis (gfx950): ursn_cluster_profile sorts the members of every cluster into
// segments (bins) of `step` voxels along the axis of its object record and reduces each bin to a count, a fixed-point charge and a
// coordinate sum around the record's anchor, then derives per-bin centroids and dQ/dx and a per-row record (filled bins, gaps, the
// charge at either end, the polyline through the centroids and its sharpest bend).  include/uresnet_hip.h names the columns;
// uresnet_amd/clusters.py (cluster_profile_numpy) states every field operation by operation, and this file follows it: the same bits.
//
// Why the bits do not move.  A member's bin is a function of that member and its row's object record alone (the fp32 projection of
// cluster_features.hip, then three fp64 operations), so it does not depend on any other thread.  Everything accumulated is a 64-bit
// INTEGER (atomic add at agent scope, atomic or for the flag): the sums are exact in any order and in any grouping.  Bounds with
// every extent <= 32768 and fewer than 2^31 entries: bin n < 2^31, |d| < 2^15 * 2^31 = 2^46, |rint(value * 2^16)| <= 2^31 so
// |charge| <= 2^62, at most 65536 bins per row and fewer than 2^31 in all.  Everything in fp64 is computed by ONE thread per bin or
// per row in a fixed order under contract(off); fp64 divide and sqrt are correctly rounded on this device.  No float atomics.
//
// Contention.  The list is sorted by index, so neighbouring entries mostly share (row, bin).  A workgroup takes PF_ROUNDS * 256
// consecutive entries.  In each round the lanes of a wave that hold the same bin next to each other are combined by a segmented
// shuffle reduction (runs by ballot); the first lane of each run adds the run to a 256-slot table of the workgroup in LDS (open
// addressing on the global bin, 64-bit integer LDS atomics); a run that finds the table full after 256 probes goes straight to
// global memory; the table is flushed once at the end: one global atomic per field and distinct bin of a workgroup.
// URSN_CLPROF_WAVE=0 keeps one global atomic set per entry, the plain route the bits are compared against.
//
// Launches: (1) per row nb_true and pad from the object record, and the status word; (2) one workgroup scans nb into bin_offsets, a
// chunk per thread, and decides the overflow; (3) clears the bins below the total; (4) the member pass; (5) one thread per bin: the
// fp64 columns; (6) one thread per row: the row record, its loop bounded by max_bins.  Every loop is bounded: the event search runs
// at most 17 halvings, the bin-to-row search at most 32, the strides end at the counts.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define PF_FI URSN_CLFEAT_I
#define PF_FR URSN_CLFEAT_R
#define PF_BI URSN_CLPROF_BI
#define PF_BR URSN_CLPROF_BR
#define PF_RI URSN_CLPROF_RI
#define PF_RR URSN_CLPROF_RR
enum { FI_N = 0, FI_M = 11, FR_AXIS = 12, FR_LEN = 15, FR_TLO = 16 };   // the object record's columns read here
enum { BI_N = 0, BI_CHARGE = 1, BI_D = 2, BI_FLAGS = 5 };
enum { ST_IDS = 1, ST_EMPTY = 2 };
#define PF_ROUNDS 2            // list entries per thread of the member pass
#define PF_SCAN_THREADS 1024
#define PF_CHUNK 8            // bins the row pass loads ahead of its walk
#define PF_GRID_CAP 4096       // workgroup cap of the striding kernels
#define PF_MAX_LENGTH 131072.0 // no object record is longer: sqrt(3) * 32768 < 2^17

typedef long long pf_i64;
typedef unsigned long long pf_u64;

struct PfArgs {
  ursn_cluster_prof_desc d;
  ursn_cluster_prof_out o;
  int S[3];          // the shape as three axes, last fastest; the coordinates of a 2-D shape are (x0, x1, 0)
  int32_t M;         // == d.m_total
  int64_t rows_max;  // min(cap_rows, feat_cap, m_total): no more rows are considered
  double* pad;       // [rows_max] scratch
  int32_t* nbt;      // [rows_max] scratch: nb_true, 0 = a skipped row
  int combine;       // 1: equal-bin lanes of a wave share one atomic set, then the workgroup's LDS table
};

__device__ __forceinline__ int64_t pf_rows(const PfArgs& a) {
  const int64_t k = a.d.table_offsets[a.d.n];
  return k < 0 ? 0 : k > a.rows_max ? a.rows_max : k;
}
__device__ __forceinline__ void pf_status(const PfArgs& a, int bits) {
  __hip_atomic_fetch_or(a.o.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Set by launch 2 alone, read by the launches behind it: uniform over a grid.
__device__ __forceinline__ bool pf_overflowed(const PfArgs& a) {
  return (__hip_atomic_load(a.o.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & URSN_CLPROF_BIN_OVERFLOW) != 0;
}
__device__ __forceinline__ void pf_add(int64_t* p, pf_i64 v) {
  if (v != 0) __hip_atomic_fetch_add((pf_i64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One bin's share -> the int64 bin table.
__device__ __forceinline__ void pf_global(const PfArgs& a, int32_t key, pf_i64 n, pf_i64 q, pf_i64 d0, pf_i64 d1, pf_i64 d2, int bad) {
  int64_t* t = a.o.bin_itab + (int64_t)key * PF_BI;
  pf_add(t + BI_N, n), pf_add(t + BI_CHARGE, q), pf_add(t + BI_D, d0), pf_add(t + BI_D + 1, d1), pf_add(t + BI_D + 2, d2);
  if (bad) __hip_atomic_fetch_or((pf_i64*)(t + BI_FLAGS), (pf_i64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A run = consecutive lanes of the wave with the same key >= 0.  Returns the lane one past the end of this lane's run and whether
// this lane is the run's first.  Every lane of the wave calls it.
__device__ __forceinline__ int pf_run(int key, int lane, bool& lead) {
  const bool act = key >= 0;
  const int up = __shfl_up(key, 1, 64);
  const bool head = act && (lane == 0 || up != key);
  const pf_u64 mh = __ballot(head), ma = __ballot(act);
  const pf_u64 above = ~((2ull << lane) - 1ull);   // lanes above this one (lane 63: none)
  const pf_u64 nb = (mh | ~ma) & above;
  lead = head;
  return act ? (nb ? __ffsll((pf_i64)nb) - 1 : 64) : lane + 1;
}
// Segmented suffix sum by doubling: after the step of distance d a lane holds its run's lanes [lane, min(lane + 2d, end)).
template <class T>
__device__ __forceinline__ T pf_seg_sum(T v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_down(v, d, 64);
    if (lane + d < end) v += o;
  }
  return v;
}

__device__ __forceinline__ void pf_coords(const PfArgs& a, int32_t idx, int ndim, int (&x)[3]) {
  const uint32_t u = (uint32_t)idx, S1 = (uint32_t)a.S[1], S2 = (uint32_t)a.S[2];
  const uint32_t q = u / S2;
  const int c2 = (int)(u - q * S2), c1 = (int)(q % S1), c0 = (int)(q / S1);
  if (ndim == 3) x[0] = c0, x[1] = c1, x[2] = c2;
  else x[0] = c1, x[1] = c2, x[2] = 0;
}

// ---- launch 1: the status word; per row nb_true and pad ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clprof_count_kernel(PfArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if (t0 == 0) *a.o.status = 0;
  const int64_t K = pf_rows(a);
  const double step = a.d.step;
  for (int64_t r = t0; r < K; r += stride) {
    const int64_t n = a.d.itab[r * PF_FI + FI_N];
    const double length = a.d.rtab[r * PF_FR + FR_LEN];
    int32_t nbt = 0;
    double pad = 0.0;
    if (n > 0 && length >= 0.0 && length <= PF_MAX_LENGTH) {   // else: not a row ursn_cluster_features wrote; launch 6 reports it
      const double q = floor(length / step);
      nbt = (int32_t)q + 1;                                    // q <= 2^17 / 0.5
      pad = ((double)nbt * step - length) / 2.0;
    }
    a.nbt[r] = nbt, a.pad[r] = pad;
  }
}

// ---- launch 2: one workgroup: the exclusive scan of nb into bin_offsets; the overflow bit ----------------------------------------------
__global__ __launch_bounds__(PF_SCAN_THREADS) void clprof_scan_kernel(PfArgs a) {
  __shared__ pf_i64 part[PF_SCAN_THREADS];
  const int64_t K = pf_rows(a);
  const int64_t per = (K + PF_SCAN_THREADS - 1) / PF_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per < K ? (int64_t)threadIdx.x * per : K, hi = lo + per < K ? lo + per : K;
  const int32_t cap = a.d.max_bins;
  pf_i64 sum = 0;
  for (int64_t r = lo; r < hi; ++r) sum += a.nbt[r] < cap ? a.nbt[r] : cap;
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < PF_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunk sums
    const pf_i64 o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += o;
    __syncthreads();
  }
  pf_i64 at = part[threadIdx.x] - sum;
  for (int64_t r = lo; r < hi; ++r) {
    a.o.bin_offsets[r] = at;
    at += a.nbt[r] < cap ? a.nbt[r] : cap;
  }
  if (threadIdx.x == PF_SCAN_THREADS - 1) {
    a.o.bin_offsets[K] = part[threadIdx.x];
    if (part[threadIdx.x] > a.o.bin_cap) pf_status(a, URSN_CLPROF_BIN_OVERFLOW);
  }
}

// ---- launch 3: the integer bins below the total -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clprof_clear_kernel(PfArgs a) {
  if (pf_overflowed(a)) return;
  const int64_t cells = a.o.bin_offsets[pf_rows(a)] * PF_BI, stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < cells; t += stride) a.o.bin_itab[t] = 0;
}

// ---- launch 4: PF_ROUNDS list entries per thread: the entry's bin, then count, charge and coordinate sums into it ------------------------
__global__ __launch_bounds__(256) void clprof_member_kernel(PfArgs a) {
  __shared__ int32_t tkey[256];
  __shared__ int32_t tbad[256];
  __shared__ pf_i64 tval[256 * 5];
  if (pf_overflowed(a)) return;
  const int lane = threadIdx.x & 63;
  const int64_t K = pf_rows(a);
  if (a.combine) {
    tkey[threadIdx.x] = -1, tbad[threadIdx.x] = 0;
#pragma unroll
    for (int f = 0; f < 5; ++f) tval[threadIdx.x * 5 + f] = 0;
    __syncthreads();
  }
  for (int round = 0; round < PF_ROUNDS; ++round) {
    const int64_t j64 = ((int64_t)blockIdx.x * PF_ROUNDS + round) * 256 + threadIdx.x;
    int key = -1, dx[3] = {0, 0, 0}, bad = 0;
    pf_i64 q = 0;
    if (j64 < a.M) {
      const int j = (int)j64;
      const int32_t id = a.d.cluster[j];
      if (id >= 0) {
        int lo = 0, hi = a.d.n - 1;
        for (int s = 0; s < 17 && lo < hi; ++s) {   // n <= 65535: at most 16 halvings
          const int mid = (lo + hi + 1) >> 1;
          if (a.d.offsets[mid] <= j) lo = mid;
          else hi = mid - 1;
        }
        const int64_t r = a.d.table_offsets[lo] + id, rend = a.d.table_offsets[lo + 1];
        const uint32_t vox = (uint32_t)a.S[0] * (uint32_t)a.S[1] * (uint32_t)a.S[2];
        const int32_t idx = a.d.index[j];
        if (lo < hi || a.d.offsets[lo] > j || j >= a.d.offsets[lo + 1] || r < 0 || r >= rend || (uint32_t)idx >= vox) {
          pf_status(a, ST_IDS);        // not a list ursn_cluster_voxels labelled
        } else if (r < K && a.nbt[r] > 0) {
          int x[3];
          pf_coords(a, idx, a.d.ndim, x);
          const int64_t* t = a.d.itab + r * PF_FI;
          const double* f = a.d.rtab + r * PF_FR;
#pragma unroll
          for (int c = 0; c < 3; ++c) dx[c] = x[c] - (int)t[FI_M + c];
          const double p0 = f[FR_AXIS + 0] * (double)dx[0];
          const double p1 = f[FR_AXIS + 1] * (double)dx[1];
          const double p2 = f[FR_AXIS + 2] * (double)dx[2];
          float tf = (float)((p0 + p1) + p2);
          if (tf == 0.f) tf = 0.f;     // -0 -> +0
          const int64_t base = a.o.bin_offsets[r];
          const int nb = (int)(a.o.bin_offsets[r + 1] - base);
          const double u = (((double)tf - f[FR_TLO]) + a.pad[r]) / a.d.step;
          const double fl = floor(u);
          const int b = fl >= (double)(nb - 1) ? nb - 1 : fl >= 0.0 ? (int)fl : 0;   // a NaN (no object record gives one): bin 0
          key = (int)(base + b);       // below the total <= bin_cap < 2^31
          if (a.d.value) {
            const float v = a.d.value[j];
            if (fabsf(v) < 32768.f) q = (pf_i64)rint((double)v * 65536.0);
            else bad = 1;              // too large for the fixed point, infinite or NaN
          }
        }
      }
    }
    if (!a.combine) {
      if (key >= 0) pf_global(a, key, 1, q, dx[0], dx[1], dx[2], bad);
      continue;
    }
    bool lead;
    const int end = pf_run(key, lane, lead);
    const pf_i64 cnt = end - lane;
    const pf_i64 sq = pf_seg_sum(q, lane, end);
    const int s0 = pf_seg_sum(dx[0], lane, end), s1 = pf_seg_sum(dx[1], lane, end), s2 = pf_seg_sum(dx[2], lane, end);   // <= 64 * 32767
    const int sb = pf_seg_sum(bad, lane, end);
    if (lead) {
      uint32_t slot = ((uint32_t)key * 2654435761u) >> 24;
      bool placed = false;
      for (int probe = 0; probe < 256 && !placed; ++probe) {
        const int32_t old = atomicCAS(&tkey[slot], -1, key);
        if (old == -1 || old == key) placed = true;
        else slot = (slot + 1) & 255;
      }
      if (placed) {
        pf_i64* v = tval + slot * 5;
        __hip_atomic_fetch_add(v + 0, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (sq) __hip_atomic_fetch_add(v + 1, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (s0) __hip_atomic_fetch_add(v + 2, (pf_i64)s0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (s1) __hip_atomic_fetch_add(v + 3, (pf_i64)s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (s2) __hip_atomic_fetch_add(v + 4, (pf_i64)s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (sb) __hip_atomic_fetch_or(&tbad[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {   // the table holds 256 other bins: the run still arrives
        pf_global(a, key, cnt, sq, s0, s1, s2, sb);
      }
    }
  }
  if (!a.combine) return;
  __syncthreads();
  const int32_t key = tkey[threadIdx.x];
  if (key >= 0) {
    const pf_i64* v = tval + threadIdx.x * 5;
    pf_global(a, key, v[0], v[1], v[2], v[3], v[4], tbad[threadIdx.x]);
  }
}

// ---- launch 5: one thread per bin: centroid and dQ/dx -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clprof_bin_kernel(PfArgs a) {
  if (pf_overflowed(a)) return;
  const int64_t K = pf_rows(a), stride = (int64_t)gridDim.x * 256;
  if (K == 0) return;
  const int64_t total = a.o.bin_offsets[K];
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += stride) {
    int64_t lo = 0, hi = K - 1;                     // the last row whose first bin is at or before g: the row that holds g
    for (int s = 0; s < 32 && lo < hi; ++s) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.o.bin_offsets[mid] <= g) lo = mid;
      else hi = mid - 1;
    }
    const int64_t* t = a.o.bin_itab + g * PF_BI;
    double* f = a.o.bin_rtab + g * PF_BR;
    const int64_t n = t[BI_N];
    if (n <= 0) {
      f[0] = f[1] = f[2] = f[3] = 0.0;
      continue;
    }
    const double fn = (double)n;
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = (double)a.d.itab[lo * PF_FI + FI_M + c] + (double)t[BI_D + c] / fn;
    f[3] = ((double)t[BI_CHARGE] / 65536.0) / a.d.step;
  }
}

// ---- launch 6: one thread per row: the row record -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void clprof_row_kernel(PfArgs a) {
  if (pf_overflowed(a)) return;
  const int64_t K = pf_rows(a), stride = (int64_t)gridDim.x * 64;
  const double step = a.d.step;
  for (int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x; r < K; r += stride) {
    int64_t* ri = a.o.row_itab + r * PF_RI;
    double* rr = a.o.row_rtab + r * PF_RR;
    const int32_t nbt = a.nbt[r];
    if (nbt <= 0) {                                  // skipped: no bins, an empty record
      pf_status(a, a.d.itab[r * PF_FI + FI_N] <= 0 ? ST_EMPTY : ST_IDS);
      for (int c = 0; c < PF_RI; ++c) ri[c] = 0;
      for (int c = 0; c < PF_RR; ++c) rr[c] = 0.0;
      continue;
    }
    const int64_t base = a.o.bin_offsets[r];
    int nb = (int)(a.o.bin_offsets[r + 1] - base);
    if (nb > a.d.max_bins) nb = a.d.max_bins;        // it is not: the loop bound in so many words
    const int h = a.d.end_bins < nb / 2 ? a.d.end_bins : nb / 2;
    pf_i64 filled = 0, gaps = 0, longest = 0, run = 0, peak = 0, peakq = 0, head_n = 0, head_q = 0, tail_n = 0, tail_q = 0, flags = 0;
    bool seen = false, have_seg = false, have_best = false;
    double path = 0.0, best = 1.0, kink = -1.0;
    double pc0 = 0.0, pc1 = 0.0, pc2 = 0.0, pd0 = 0.0, pd1 = 0.0, pd2 = 0.0, ps = 0.0;
    int pb = 0;
    // PF_CHUNK bins are loaded at once (their addresses do not depend on the walk), then walked in order from registers: the loop is
    // a chain of dependent steps, and one global load latency per bin would dominate a long track.
    for (int b0 = 0; b0 < nb; b0 += PF_CHUNK) {
      pf_i64 ln[PF_CHUNK], lq[PF_CHUNK], lf[PF_CHUNK];
      double lc[PF_CHUNK][3];
#pragma unroll
      for (int k = 0; k < PF_CHUNK; ++k) {
        const int64_t g = base + (b0 + k < nb ? b0 + k : nb - 1);   // clamped: always a bin of this row
        const int64_t* t = a.o.bin_itab + g * PF_BI;
        const double* f = a.o.bin_rtab + g * PF_BR;
        ln[k] = t[BI_N], lq[k] = t[BI_CHARGE], lf[k] = t[BI_FLAGS];
        lc[k][0] = f[0], lc[k][1] = f[1], lc[k][2] = f[2];
      }
#pragma unroll
      for (int k = 0; k < PF_CHUNK; ++k) {
        const int b = b0 + k;
        if (b >= nb) break;
        const pf_i64 n = ln[k], q = lq[k];
        flags |= lf[k] & 1;
        if (b == 0 || q > peakq) peak = b, peakq = q;
        if (b < h) head_n += n, head_q += q;
        if (b >= nb - h) tail_n += n, tail_q += q;
        if (n <= 0) {
          ++run;
          continue;
        }
        ++filled;
        if (seen && run > 0) {
          ++gaps;
          if (run > longest) longest = run;
        }
        run = 0;
        const double c0 = lc[k][0], c1 = lc[k][1], c2 = lc[k][2];
        if (seen) {
          const double d0 = c0 - pc0, d1 = c1 - pc1, d2 = c2 - pc2;
          const double s = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
          path = path + s;
          if (have_seg) {
            const double den = ps * s;
            if (den != 0.0) {
              const double cs = ((pd0 * d0 + pd1 * d1) + pd2 * d2) / den;
              if (!have_best || cs < best) best = cs, kink = (double)pb, have_best = true;
            }
          }
          pd0 = d0, pd1 = d1, pd2 = d2, ps = s, have_seg = true;
        }
        pc0 = c0, pc1 = c1, pc2 = c2, pb = b, seen = true;
      }
    }
    if (nbt > a.d.max_bins) flags |= 2;
    ri[0] = nb, ri[1] = filled, ri[2] = gaps, ri[3] = longest, ri[4] = peak, ri[5] = h;
    ri[6] = head_n, ri[7] = head_q, ri[8] = tail_n, ri[9] = tail_q;
    ri[10] = h == 0 ? 0 : tail_q > head_q ? 1 : tail_q < head_q ? -1 : 0;
    ri[11] = flags;
    const double length = a.d.rtab[r * PF_FR + FR_LEN];
    rr[0] = path, rr[1] = have_best ? best : 1.0, rr[2] = kink;
    if (h > 0) {
      const double den = (double)h * step;
      rr[3] = ((double)head_q / 65536.0) / den;
      rr[4] = ((double)tail_q / 65536.0) / den;
    } else {
      rr[3] = 0.0, rr[4] = 0.0;
    }
    rr[5] = path != 0.0 ? length / path : 1.0;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline int64_t pf_rows_max(int64_t m_total, int64_t cap_rows) { return cap_rows < m_total ? cap_rows : m_total; }
static inline size_t pf_up8(size_t x) { return (x + 7) & ~(size_t)7; }

extern "C" size_t ursn_cluster_profile_scratch_bytes(int32_t n, int64_t m_total, int64_t cap_rows, int64_t bin_cap) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 31) || cap_rows < 0 || bin_cap < 0 || bin_cap >= ((int64_t)1 << 31))
    return 0;
  const size_t R = (size_t)pf_rows_max(m_total, cap_rows);
  return R * sizeof(double) + pf_up8(R * sizeof(int32_t)) + 8;
}

extern "C" int ursn_cluster_profile(const ursn_cluster_prof_desc* d, const ursn_cluster_prof_out* out, void* scratch,
                                    size_t scratch_bytes, void* stream) {
  const char* who = "cluster_profile";
  URSN_REQUIRE(d && out, "%s: null desc / out", who);
  URSN_REQUIRE(d->ndim == 2 || d->ndim == 3, "%s: ndim = %d, must be 2 or 3", who, (int)d->ndim);
  int64_t vox = 1;
  for (int i = 0; i < d->ndim; ++i) {
    URSN_REQUIRE(d->spatial[i] >= 1 && d->spatial[i] <= 32768, "%s: spatial[%d] = %d outside [1, 32768]", who, i, (int)d->spatial[i]);
    vox *= d->spatial[i];
  }
  URSN_REQUIRE(vox < ((int64_t)1 << 31), "%s: prod(spatial) >= 2^31 (indices are int32)", who);
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)d->n);
  URSN_REQUIRE(d->m_total >= 0 && d->m_total < ((int64_t)1 << 31), "%s: m_total = %lld outside [0, 2^31)", who,
               (long long)d->m_total);
  URSN_REQUIRE(d->step >= 0.5 && d->step <= 4096.0, "%s: step = %g outside [0.5, 4096]", who, d->step);   // a NaN fails both
  URSN_REQUIRE(d->end_bins >= 1 && d->end_bins <= 16, "%s: end_bins = %d outside [1, 16]", who, (int)d->end_bins);
  URSN_REQUIRE(d->max_bins >= 1 && d->max_bins <= 65536, "%s: max_bins = %d outside [1, 65536]", who, (int)d->max_bins);
  URSN_REQUIRE(d->feat_cap >= 0, "%s: feat_cap = %lld < 0", who, (long long)d->feat_cap);
  URSN_REQUIRE(out->cap_rows >= 0, "%s: cap_rows = %lld < 0", who, (long long)out->cap_rows);
  URSN_REQUIRE(out->bin_cap >= 0 && out->bin_cap < ((int64_t)1 << 31), "%s: bin_cap = %lld outside [0, 2^31)", who,
               (long long)out->bin_cap);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster), "%s: null index / cluster", who);
  URSN_REQUIRE(d->feat_cap == 0 || (d->itab && d->rtab), "%s: null itab / rtab", who);
  URSN_REQUIRE(out->status && out->bin_offsets, "%s: null out->status / out->bin_offsets", who);
  URSN_REQUIRE(out->cap_rows == 0 || (out->row_itab && out->row_rtab), "%s: null out->row_itab / out->row_rtab", who);
  URSN_REQUIRE(out->bin_cap == 0 || (out->bin_itab && out->bin_rtab), "%s: null out->bin_itab / out->bin_rtab", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)d->itab | (uintptr_t)d->rtab |
                 (uintptr_t)out->bin_offsets | (uintptr_t)out->bin_itab | (uintptr_t)out->bin_rtab | (uintptr_t)out->row_itab |
                 (uintptr_t)out->row_rtab | (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->value | (uintptr_t)d->cluster | (uintptr_t)out->status) & 3) == 0,
               "%s: index / value / cluster / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_profile_scratch_bytes(d->n, d->m_total, out->cap_rows, out->bin_cap);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  PfArgs a;
  a.d = *d;
  a.o = *out;
  if (d->ndim == 3) a.S[0] = d->spatial[0], a.S[1] = d->spatial[1], a.S[2] = d->spatial[2];
  else a.S[0] = 1, a.S[1] = d->spatial[0], a.S[2] = d->spatial[1];
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  const int64_t R = pf_rows_max(M, out->cap_rows);   // the scratch is laid out for R rows
  a.rows_max = R < d->feat_cap ? R : d->feat_cap;
  a.pad = (double*)scratch;
  a.nbt = (int32_t*)((char*)scratch + (size_t)R * sizeof(double));
  a.combine = ursn_env_on("URSN_CLPROF_WAVE") ? 1 : 0;   // read at every call: the two routes are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const auto blocks = [](int64_t items, int per) {
    const int64_t b = cdiv64(items, per);
    return dim3((unsigned)(b < 1 ? 1 : b > PF_GRID_CAP ? PF_GRID_CAP : b));
  };
  ursn_note_kernel("clprof_count");
  hipLaunchKernelGGL(clprof_count_kernel, blocks(a.rows_max, 256), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clprof_scan");
  hipLaunchKernelGGL(clprof_scan_kernel, dim3(1), dim3(PF_SCAN_THREADS), 0, s, a);
  URSN_HIP(hipGetLastError());
  if (a.rows_max == 0) return 0;   // no row is considered: bin_offsets[0] and the status are written
  ursn_note_kernel("clprof_clear");
  hipLaunchKernelGGL(clprof_clear_kernel, blocks(out->bin_cap * PF_BI, 256), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clprof_member");
  hipLaunchKernelGGL(clprof_member_kernel, dim3((unsigned)cdiv64(M, 256 * PF_ROUNDS)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clprof_bin");
  hipLaunchKernelGGL(clprof_bin_kernel, blocks(out->bin_cap, 256), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clprof_row");
  hipLaunchKernelGGL(clprof_row_kernel, blocks(a.rows_max, 64), dim3(64), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
