// Cluster matching (gfx950): ursn_cluster_match builds the contingency table of two clusterings of the same voxel lists and reduces
// it to one record per row of either side, one per event and, on request, the list of cells.  include/uresnet_hip.h names the
// columns; uresnet_amd/clusters.py (cluster_match_numpy) states every field operation by operation, and this file follows it: the
// same bits.
//
// One keyed reduction.  Every list entry has a PAIR (global A row, global B row); a side whose id is -1 holds the marker NONE, so an
// entry in a row of one side only still has a pair of its own kind, and an entry in no row has none.  The pairs are counted in an
// open-addressing table in the scratch: 2^k >= 2 max(m_total, 1) slots, the key (A row << 32) | B row claimed with a 64-bit
// compare-and-swap from the EMPTY key the first launch writes, then count (+ dropped charges << 32) and fixed-point charge added
// with 64-bit integer atomics.  At most m_total distinct pairs exist, so the load never passes 1/2; a probe walk is capped at the
// slot count and sets *status if it runs out.  Which slot a pair lands in depends on arrival order; everything below reads the
// table as a SET.  A pass over the slots then spreads each pair onto its rows: n, charge, dropped charges for either kind; matched,
// partners, c (c - 1) / 2 and the packed best (c << 32 | 0xFFFFFFFF - other row, one 64-bit atomic max: equal counts fall to the
// lower row) for a cell.  All of it integer adds and maxima: exact whatever the order.  One thread per row writes the record (the
// best cell's charge is looked up in the table, the other side's n and best are complete by then), and adds the row's share of the
// event sums; rows of an event are neighbours, so a wave combines them per event first.  Everything in fp64 is computed by ONE
// thread in a fixed order under contract(off).
//
// Contention.  Neighbouring list entries nearly always share their pair.  The lanes of a wave that hold the same pair next to each
// other are combined by a segmented shuffle reduction, the first lane of each run adds the run to a 256-slot table of the workgroup
// in LDS (open addressing on the pair; at most 256 runs per workgroup, so it cannot fill up and a probe walk is capped at 256), and
// each distinct pair of the workgroup then costs ONE insertion into the global table.  URSN_CLMATCH_WAVE=0 keeps one insertion per
// entry, the plain route the bits are compared against.
//
// Launches: init (status, slots, the rows below the device-read counts, event sums), per-entry insertion, slot pass, A rows, B rows,
// event records; with a cell list: scan of partners, drop into the segments, rank.  Every loop is bounded.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define CM_I URSN_CLMATCH_I
#define CM_R URSN_CLMATCH_R
#define CM_EI URSN_CLMATCH_EI
#define CM_ER URSN_CLMATCH_ER
enum { RW_N = 0, RW_CHARGE = 1, RW_MATCHED = 2, RW_PARTNERS = 3, RW_PAIRSUM = 4, RW_BEST = 5, RW_BAD = 6, RW_CURSOR = 7, RW = 8 };
enum { EV_N = 0, EV_S = 1, EV_SA = 2, EV_SB = 3, EV_CELLS = 4, EV_KA = 5, EV_KB = 6, EV_MUTUAL = 7, EV_OVA = 8, EV_NA = 9, EV_OVB = 10,
       EV_NB = 11 };
#define CM_GRID_CAP 16384    // workgroup cap of the striding kernels
#define CM_SCAN_THREADS 1024

typedef long long cm_i64;
typedef unsigned long long cm_u64;
#define CM_EMPTY (~0ull)
#define CM_NONE 0xFFFFFFFFu

struct CmArgs {
  ursn_cluster_match_desc d;
  ursn_cluster_match_out o;
  int32_t M;          // == d.m_total
  int64_t T;          // slots, a power of two
  int shift;          // 64 - log2(T)
  cm_u64* key;        // [T]
  cm_i64* cb;         // [T] count | dropped charges << 32
  cm_i64* q;          // [T]
  cm_i64* row[2];     // [max(M, 1)][RW] per side
  int64_t* scan;      // [max(M, 1) + 1] exclusive scan of the A rows' partners
  int32_t* seg;       // [max(M, 1)] slot of each cell, by A row, unordered inside a row
  int combine;        // 1: equal-pair lanes of a wave, then the runs of a workgroup, share one insertion
};

__device__ __forceinline__ void cm_add(cm_i64* p, cm_i64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cm_umax(cm_i64* p, cm_u64 v) {
  __hip_atomic_fetch_max((cm_u64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows of a side that can have a member: the device-read count, never more than the list could fill (the scratch holds M rows).
__device__ __forceinline__ int64_t cm_rows(const int64_t* toff, int n, int32_t M) {
  const int64_t k = toff[n];
  return k < 0 ? 0 : k > M ? M : k;
}

// The largest e in [0, n) with off[e] <= x: n <= 65535, at most 16 halvings.
__device__ __forceinline__ int cm_search(const int64_t* off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  for (int s = 0; s < 17 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int64_t cm_slot(const CmArgs& a, cm_u64 key) { return (int64_t)((key * 0x9E3779B97F4A7C15ull) >> a.shift); }

// count / charge of one pair -> the global table
__device__ __forceinline__ void cm_insert(const CmArgs& a, cm_u64 key, cm_i64 cb, cm_i64 q) {
  int64_t slot = cm_slot(a, key);
  for (int64_t probe = 0; probe < a.T; ++probe) {
    cm_u64 old = __hip_atomic_load(&a.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == CM_EMPTY) {
      cm_u64 expect = CM_EMPTY;
      __hip_atomic_compare_exchange_strong(&a.key[slot], &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      old = expect == CM_EMPTY ? key : expect;
    }
    if (old == key) {
      cm_add(&a.cb[slot], cb);
      if (q) cm_add(&a.q[slot], q);
      return;
    }
    slot = (slot + 1) & (a.T - 1);
  }
  *a.o.status = 3;   // cannot happen: at most M distinct pairs in >= 2 M slots
}

// the slot of a pair that is in the table, or -1
__device__ __forceinline__ int64_t cm_find(const CmArgs& a, cm_u64 key) {
  int64_t slot = cm_slot(a, key);
  for (int64_t probe = 0; probe < a.T; ++probe) {
    const cm_u64 k = a.key[slot];
    if (k == key) return slot;
    if (k == CM_EMPTY) return -1;
    slot = (slot + 1) & (a.T - 1);
  }
  return -1;
}

// A run = consecutive lanes of the wave with the same key (64-bit pairs, or events as small integers; `none` = no key).  Returns the
// lane one past the end of this lane's run and whether this lane is the run's first.  Without combining every active lane is its own run.
__device__ __forceinline__ int cm_run(cm_u64 key, cm_u64 none, int lane, int combine, bool& lead) {
  const bool act = key != none;
  if (!combine) {
    lead = act;
    return lane + 1;
  }
  const cm_u64 up = __shfl_up(key, 1, 64);
  const bool head = act && (lane == 0 || up != key);
  const cm_u64 mh = __ballot(head), ma = __ballot(act);
  const cm_u64 above = ~((2ull << lane) - 1ull);   // lanes above this one (lane 63: none)
  const cm_u64 nb = (mh | ~ma) & above;
  lead = head;
  return act ? (nb ? __ffsll((cm_i64)nb) - 1 : 64) : lane + 1;
}

// Segmented suffix sum by doubling: after the step of distance d a lane holds its run's lanes [lane, min(lane + 2d, end)).  Every
// lane of the wave calls it; `combine` is uniform.
__device__ __forceinline__ cm_i64 cm_seg_sum(cm_i64 v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const cm_i64 o = __shfl_down(v, d, 64);
      if (lane + d < end) v += o;
    }
  }
  return v;
}

// ---- launch 1: status, the empty table, the rows below the counts, the event sums ---------------------------------------------------
__global__ __launch_bounds__(256) void clmatch_init_kernel(CmArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int n = a.d.n;
  if (t0 == 0) {
    const int64_t ka = a.d.table_offsets_a[n], kb = a.d.table_offsets_b[n];
    *a.o.status = (ka < 0 || ka > a.M || kb < 0 || kb > a.M || a.d.table_offsets_a[0] != 0 || a.d.table_offsets_b[0] != 0 ||
                   a.d.offsets[0] != 0 || a.d.offsets[n] != a.M) ? 1 : 0;   // more rows than entries: one has no member
  }
  for (int64_t t = t0; t < a.T; t += step) a.key[t] = CM_EMPTY, a.cb[t] = 0, a.q[t] = 0;
  const int64_t wa = cm_rows(a.d.table_offsets_a, n, a.M) * RW, wb = cm_rows(a.d.table_offsets_b, n, a.M) * RW;
  for (int64_t t = t0; t < wa; t += step) a.row[0][t] = 0;
  for (int64_t t = t0; t < wb; t += step) a.row[1][t] = 0;
  for (int64_t t = t0; t < (int64_t)n * CM_EI; t += step) a.o.event_int[t] = 0;
}

// ---- launch 2: one thread per list entry: its pair into the table ---------------------------------------------------------------------
__device__ __forceinline__ bool cm_row_of(const int64_t* toff, int e, int32_t id, int64_t rows, uint32_t& r) {
  if (id < 0) return id == -1;         // -1: no row on this side (r stays NONE)
  const int64_t g = toff[e] + id;
  if (g < 0 || g >= toff[e + 1] || g >= rows) return false;
  r = (uint32_t)g;
  return true;
}

__global__ __launch_bounds__(256) void clmatch_entry_kernel(CmArgs a) {
  __shared__ cm_u64 tkey[256];
  __shared__ cm_i64 tcb[256], tq[256];
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  cm_u64 key = CM_EMPTY;
  cm_i64 q = 0, bad = 0;
  if (j64 < a.M) {
    const int j = (int)j64;
    const int32_t ia = a.d.cluster_a[j], ib = a.d.cluster_b[j];
    if (ia != -1 || ib != -1) {
      const int e = cm_search(a.d.offsets, a.d.n, j);
      uint32_t ra = CM_NONE, rb = CM_NONE;
      if (a.d.offsets[e] > j || j >= a.d.offsets[e + 1] ||
          !cm_row_of(a.d.table_offsets_a, e, ia, cm_rows(a.d.table_offsets_a, a.d.n, a.M), ra) ||
          !cm_row_of(a.d.table_offsets_b, e, ib, cm_rows(a.d.table_offsets_b, a.d.n, a.M), rb)) {
        *a.o.status = 1;               // not ids ursn_cluster_voxels wrote for these lists: the entry is skipped
      } else {
        key = ((cm_u64)ra << 32) | rb;
        if (a.d.value) {
          const float v = a.d.value[j];
          if (fabsf(v) < 32768.f) q = (cm_i64)rint((double)v * 65536.0);
          else bad = 1;                // too large for the fixed point, infinite or NaN
        }
      }
    }
  }
  if (!a.combine) {
    if (key != CM_EMPTY) cm_insert(a, key, 1 | (bad << 32), q);
    return;
  }
  bool lead;
  const int end = cm_run(key, CM_EMPTY, lane, 1, lead);
  const cm_i64 cb = (cm_i64)(end - lane) | (cm_seg_sum(bad, lane, end, 1) << 32);
  q = cm_seg_sum(q, lane, end, 1);
  tkey[threadIdx.x] = CM_EMPTY, tcb[threadIdx.x] = 0, tq[threadIdx.x] = 0;
  __syncthreads();
  if (lead) {
    uint32_t slot = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 56);
    bool placed = false;
    for (int probe = 0; probe < 256 && !placed; ++probe) {
      const cm_u64 old = atomicCAS(&tkey[slot], CM_EMPTY, key);
      if (old == CM_EMPTY || old == key) placed = true;
      else slot = (slot + 1) & 255;
    }
    if (placed) {
      __hip_atomic_fetch_add(&tcb[slot], cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (q) __hip_atomic_fetch_add(&tq[slot], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {   // cannot happen (at most 256 runs, 256 slots); the totals still arrive
      cm_insert(a, key, cb, q);
    }
  }
  __syncthreads();
  const cm_u64 k = tkey[threadIdx.x];
  if (k != CM_EMPTY) cm_insert(a, k, tcb[threadIdx.x], tq[threadIdx.x]);
}

// ---- launch 3: one thread per slot: an occupied one spreads its pair onto its rows ------------------------------------------------------
__device__ __forceinline__ void cm_spread(cm_i64* row, cm_i64 c, cm_i64 nbad, cm_i64 q, bool cell, uint32_t other) {
  cm_add(row + RW_N, c);
  if (q) cm_add(row + RW_CHARGE, q);
  if (nbad) cm_add(row + RW_BAD, nbad);
  if (cell) {
    cm_add(row + RW_MATCHED, c);
    cm_add(row + RW_PARTNERS, 1);
    if (c > 1) cm_add(row + RW_PAIRSUM, c * (c - 1) / 2);
    cm_umax(row + RW_BEST, ((cm_u64)c << 32) | (cm_u64)(0xFFFFFFFFu - other));
  }
}

__global__ __launch_bounds__(256) void clmatch_slot_kernel(CmArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256;
  const int64_t RA = cm_rows(a.d.table_offsets_a, a.d.n, a.M), RB = cm_rows(a.d.table_offsets_b, a.d.n, a.M);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += step) {
    const cm_u64 key = a.key[t];
    if (key == CM_EMPTY) continue;
    const uint32_t ra = (uint32_t)(key >> 32), rb = (uint32_t)key;
    const cm_i64 cb = a.cb[t], c = cb & 0xFFFFFFFFll, nbad = cb >> 32, q = a.q[t];
    const bool cell = ra != CM_NONE && rb != CM_NONE;
    if (ra != CM_NONE && ra < RA) cm_spread(a.row[0] + (int64_t)ra * RW, c, nbad, q, cell, rb);
    if (rb != CM_NONE && rb < RB) cm_spread(a.row[1] + (int64_t)rb * RW, c, nbad, q, cell, ra);
  }
}

// ---- launches 4 and 5: one thread per row of side X: its record and its share of the event sums -----------------------------------------
template <int X>
__global__ __launch_bounds__(256) void clmatch_row_kernel(CmArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t* toff = X == 0 ? a.d.table_offsets_a : a.d.table_offsets_b;
  const int64_t* toff_y = X == 0 ? a.d.table_offsets_b : a.d.table_offsets_a;
  const int64_t R = cm_rows(toff, a.d.n, a.M), RY = cm_rows(toff_y, a.d.n, a.M);
  const int64_t cap = X == 0 ? a.o.cap_a : a.o.cap_b;
  int64_t* itab = X == 0 ? a.o.a_int : a.o.b_int;
  double* rtab = X == 0 ? a.o.a_real : a.o.b_real;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < R; base += step) {   // uniform per workgroup: the shuffles need all lanes
    const int64_t r = base + threadIdx.x;
    int e = -1;
    cm_i64 n = 0, matched = 0, partners = 0, pairsum = 0, overlap = 0, mutual = 0;
    if (r < R) {
      const cm_i64* row = a.row[X] + r * RW;
      n = row[RW_N], matched = row[RW_MATCHED], partners = row[RW_PARTNERS], pairsum = row[RW_PAIRSUM];
      const cm_i64 charge = row[RW_CHARGE], nbad = row[RW_BAD];
      e = cm_search(toff, a.d.n, r);
      cm_i64 best = -1, oq = 0, ny = 0;
      if (toff[e] > r || r >= toff[e + 1]) {
        *a.o.status = 1, e = -1;       // table offsets that do not increase
      } else if (n <= 0) {
        *a.o.status = 2, e = -1;       // a row without members: not a table ursn_cluster_voxels wrote
        n = matched = partners = pairsum = 0;
      } else if (partners > 0) {
        const cm_u64 packed = (cm_u64)row[RW_BEST];
        const uint32_t ry = 0xFFFFFFFFu - (uint32_t)packed;
        overlap = (cm_i64)(packed >> 32);
        if (ry < RY) {
          const cm_i64* other = a.row[1 - X] + (int64_t)ry * RW;
          ny = other[RW_N];
          mutual = (0xFFFFFFFFu - (uint32_t)(cm_u64)other[RW_BEST]) == (uint32_t)r && other[RW_PARTNERS] > 0 ? 1 : 0;
          best = (cm_i64)ry - toff_y[e];
          const int64_t slot = cm_find(a, X == 0 ? ((cm_u64)(uint32_t)r << 32) | ry : ((cm_u64)ry << 32) | (uint32_t)r);
          if (slot >= 0) oq = a.q[slot];
          else *a.o.status = 3;
        } else {
          *a.o.status = 3, overlap = 0, partners = 0;
        }
      }
      if (r < cap) {
        int64_t* t = itab + r * CM_I;
        double* f = rtab + r * CM_R;
        t[0] = n, t[1] = charge, t[2] = matched, t[3] = partners, t[4] = best, t[5] = overlap, t[6] = oq;
        t[7] = (nbad > 0 ? 1 : 0) | (mutual ? 2 : 0);
        const bool cell = partners > 0 && ny > 0;
        f[0] = n > 0 ? (double)overlap / (double)n : 0.0;
        f[1] = cell ? (double)overlap / (double)ny : 0.0;
        f[2] = cell ? (double)overlap / (double)(n + ny - overlap) : 0.0;
        f[3] = n > 0 ? (double)matched / (double)n : 0.0;
      }
    }
    bool lead;
    const int end = cm_run((cm_u64)(cm_i64)e, (cm_u64)(cm_i64)-1, lane, a.combine, lead);
    const cm_i64 msum = matched * (matched - 1) / 2;
    if (X == 0) {
      const cm_i64 v[7] = {matched, pairsum, msum, partners, mutual, overlap, n};
      const int col[7] = {EV_N, EV_S, EV_SA, EV_CELLS, EV_MUTUAL, EV_OVA, EV_NA};
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const cm_i64 s = cm_seg_sum(v[k], lane, end, a.combine);
        if (lead && s) cm_add((cm_i64*)a.o.event_int + (int64_t)e * CM_EI + col[k], s);
      }
    } else {
      const cm_i64 v[3] = {msum, overlap, n};
      const int col[3] = {EV_SB, EV_OVB, EV_NB};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const cm_i64 s = cm_seg_sum(v[k], lane, end, a.combine);
        if (lead && s) cm_add((cm_i64*)a.o.event_int + (int64_t)e * CM_EI + col[k], s);
      }
    }
  }
}

// ---- launch 6: one thread per event: the counts and the fp64 columns ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void clmatch_event_kernel(CmArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.d.n) return;
  int64_t* t = a.o.event_int + (int64_t)e * CM_EI;
  double* f = a.o.event_real + (int64_t)e * CM_ER;
  int64_t ka = a.d.table_offsets_a[e + 1] - a.d.table_offsets_a[e], kb = a.d.table_offsets_b[e + 1] - a.d.table_offsets_b[e];
  if (ka < 0 || kb < 0 || ka > a.M || kb > a.M) *a.o.status = 1, ka = kb = 0;
  t[EV_KA] = ka, t[EV_KB] = kb;
  const int64_t N = t[EV_N], S = t[EV_S], SA = t[EV_SA], SB = t[EV_SB];
  const int64_t P = N * (N - 1) / 2;
  double ari = 1.0;
  if (P != 0) {
    const double E = ((double)SA * (double)SB) / (double)P;
    const double mean = ((double)SA + (double)SB) * 0.5;
    const double den = mean - E;
    if (den != 0.0) ari = ((double)S - E) / den;
  }
  f[0] = ari;
  f[1] = t[EV_NA] != 0 ? (double)t[EV_OVA] / (double)t[EV_NA] : 0.0;
  f[2] = t[EV_NB] != 0 ? (double)t[EV_OVB] / (double)t[EV_NB] : 0.0;
  f[3] = ka + kb != 0 ? (double)(2 * t[EV_MUTUAL]) / (double)(ka + kb) : 0.0;
}

// ---- launch 7: one workgroup: exclusive scan of the A rows' partners ----------------------------------------------------------------------
__global__ __launch_bounds__(CM_SCAN_THREADS) void clmatch_scan_kernel(CmArgs a) {
  __shared__ cm_i64 part[CM_SCAN_THREADS];
  const int64_t R = cm_rows(a.d.table_offsets_a, a.d.n, a.M);
  const int64_t per = (R + CM_SCAN_THREADS - 1) / CM_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < R ? lo + per : R;
  cm_i64 sum = 0;
  for (int64_t r = lo; r < hi; ++r) sum += a.row[0][r * RW + RW_PARTNERS];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < CM_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunk sums
    const cm_i64 o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += o;
    __syncthreads();
  }
  cm_i64 at = part[threadIdx.x] - sum;
  for (int64_t r = lo; r < hi; ++r) {
    a.scan[r] = at;
    if (r <= a.o.cap_a) a.o.pair_offsets[r] = at;
    at += a.row[0][r * RW + RW_PARTNERS];
  }
  if (threadIdx.x == CM_SCAN_THREADS - 1) {
    a.scan[R] = part[threadIdx.x];
    if (R <= a.o.cap_a) a.o.pair_offsets[R] = part[threadIdx.x];
  }
}

// ---- launch 8: one thread per slot: a cell drops its slot into its row's segment ------------------------------------------------------------
__global__ __launch_bounds__(256) void clmatch_drop_kernel(CmArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256;
  const int64_t RA = cm_rows(a.d.table_offsets_a, a.d.n, a.M);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += step) {
    const cm_u64 key = a.key[t];
    if (key == CM_EMPTY) continue;
    const uint32_t ra = (uint32_t)(key >> 32), rb = (uint32_t)key;
    if (ra == CM_NONE || rb == CM_NONE || ra >= RA) continue;
    cm_i64* row = a.row[0] + (int64_t)ra * RW;
    const cm_i64 pos = __hip_atomic_fetch_add(row + RW_CURSOR, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const cm_i64 at = a.scan[ra] + pos;
    if (pos < 0 || pos >= row[RW_PARTNERS] || at < 0 || at >= a.M) *a.o.status = 4;
    else a.seg[at] = (int32_t)t;       // T <= 2^32 slots: the slot as its low 32 bits
  }
}

// ---- launch 9: one thread per cell: its rank by B row inside its segment, then the cell itself ----------------------------------------------
__global__ __launch_bounds__(256) void clmatch_rank_kernel(CmArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256;
  const int64_t RA = cm_rows(a.d.table_offsets_a, a.d.n, a.M);
  int64_t total = a.scan[RA];
  if (total > a.M) total = a.M;
  for (int64_t ci = (int64_t)blockIdx.x * 256 + threadIdx.x; ci < total; ci += step) {
    const int64_t t = (int64_t)(uint32_t)a.seg[ci];
    if (t >= a.T) continue;
    const cm_u64 key = a.key[t];
    const uint32_t ra = (uint32_t)(key >> 32), rb = (uint32_t)key;
    if (key == CM_EMPTY || ra >= RA || rb == CM_NONE) { *a.o.status = 4; continue; }
    const int64_t s0 = a.scan[ra];
    int64_t cnt = a.row[0][(int64_t)ra * RW + RW_PARTNERS];
    if (ci < s0 || ci >= s0 + cnt || s0 + cnt > a.M) { *a.o.status = 4; continue; }
    int64_t rank = 0;
    for (int64_t k = 0; k < cnt; ++k) {   // bounded by partners
      const int64_t u = (int64_t)(uint32_t)a.seg[s0 + k];
      if (u < a.T && (uint32_t)a.key[u] < rb) ++rank;
    }
    const int64_t at = s0 + rank;
    if (at < a.o.pair_cap) {
      const int e = cm_search(a.d.table_offsets_a, a.d.n, ra);
      a.o.pair_b[at] = (int32_t)((int64_t)rb - a.d.table_offsets_b[e]);
      a.o.pair_n[at] = a.cb[t] & 0xFFFFFFFFll;
      a.o.pair_q[at] = a.q[t];
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int64_t cm_slots(int64_t m_total) {
  int64_t t = 2;
  while (t < 2 * (m_total < 1 ? 1 : m_total)) t <<= 1;
  return t;
}

static size_t cm_layout(int64_t m_total, CmArgs* a, char* base) {
  const size_t T = (size_t)cm_slots(m_total), M1 = (size_t)(m_total < 1 ? 1 : m_total);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 7) & ~(size_t)7; return p; };
  char* key = take(T * 8);
  char* cb = take(T * 8);
  char* q = take(T * 8);
  char* r0 = take(M1 * RW * 8);
  char* r1 = take(M1 * RW * 8);
  char* scan = take((M1 + 1) * 8);
  char* seg = take(M1 * 4);
  if (a) {
    a->key = (cm_u64*)key, a->cb = (cm_i64*)cb, a->q = (cm_i64*)q, a->row[0] = (cm_i64*)r0, a->row[1] = (cm_i64*)r1;
    a->scan = (int64_t*)scan, a->seg = (int32_t*)seg;
    a->T = (int64_t)T;
    int lg = 0;
    while (((size_t)1 << lg) < T) ++lg;
    a->shift = 64 - lg;
  }
  return off;
}

extern "C" size_t ursn_cluster_match_scratch_bytes(int32_t n, int64_t m_total, int64_t cap_a, int64_t cap_b, int64_t pair_cap) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 31) || cap_a < 0 || cap_b < 0 || pair_cap < 0) return 0;
  return cm_layout(m_total, nullptr, nullptr);
}

static unsigned cm_grid(int64_t items) {
  const int64_t b = cdiv64(items, 256);
  return (unsigned)(b < 1 ? 1 : b > CM_GRID_CAP ? CM_GRID_CAP : b);
}

extern "C" int ursn_cluster_match(const ursn_cluster_match_desc* d, const ursn_cluster_match_out* out, void* scratch,
                                  size_t scratch_bytes, void* stream) {
  const char* who = "cluster_match";
  URSN_REQUIRE(d && out, "%s: null desc / out", who);
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)d->n);
  URSN_REQUIRE(d->m_total >= 0 && d->m_total < ((int64_t)1 << 31), "%s: m_total = %lld outside [0, 2^31)", who,
               (long long)d->m_total);
  URSN_REQUIRE(out->cap_a >= 0, "%s: cap_a = %lld < 0", who, (long long)out->cap_a);
  URSN_REQUIRE(out->cap_b >= 0, "%s: cap_b = %lld < 0", who, (long long)out->cap_b);
  URSN_REQUIRE(out->pair_cap >= 0, "%s: pair_cap = %lld < 0", who, (long long)out->pair_cap);
  URSN_REQUIRE(d->offsets && d->table_offsets_a && d->table_offsets_b, "%s: null offsets / table_offsets_a / table_offsets_b", who);
  URSN_REQUIRE(d->m_total == 0 || (d->cluster_a && d->cluster_b), "%s: null cluster_a / cluster_b", who);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->event_int && out->event_real, "%s: null out->event_int / out->event_real", who);
  URSN_REQUIRE(out->cap_a == 0 || (out->a_int && out->a_real), "%s: null out->a_int / out->a_real", who);
  URSN_REQUIRE(out->cap_b == 0 || (out->b_int && out->b_real), "%s: null out->b_int / out->b_real", who);
  const int cells = (out->pair_b ? 1 : 0) + (out->pair_n ? 1 : 0) + (out->pair_q ? 1 : 0);
  URSN_REQUIRE(cells == 0 || cells == 3, "%s: out->pair_b / pair_n / pair_q must be given together or not at all", who);
  URSN_REQUIRE(cells == 0 || out->pair_offsets, "%s: the cell arrays need out->pair_offsets", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets_a | (uintptr_t)d->table_offsets_b | (uintptr_t)out->a_int |
                 (uintptr_t)out->a_real | (uintptr_t)out->b_int | (uintptr_t)out->b_real | (uintptr_t)out->event_int |
                 (uintptr_t)out->event_real | (uintptr_t)out->pair_offsets | (uintptr_t)out->pair_n | (uintptr_t)out->pair_q |
                 (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table offsets / record tables / pair_offsets / pair_n / pair_q / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->cluster_a | (uintptr_t)d->cluster_b | (uintptr_t)d->value | (uintptr_t)out->pair_b |
                 (uintptr_t)out->status) & 3) == 0,
               "%s: cluster_a / cluster_b / value / pair_b / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_match_scratch_bytes(d->n, d->m_total, out->cap_a, out->cap_b, out->pair_cap);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  CmArgs a;
  a.d = *d;
  a.o = *out;
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  cm_layout(M, &a, (char*)scratch);
  a.combine = ursn_env_on("URSN_CLMATCH_WAVE") ? 1 : 0;   // read at every call: the two routes are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const int64_t init_items = a.T > M * RW ? a.T : M * RW;
  ursn_note_kernel("clmatch_init");
  hipLaunchKernelGGL(clmatch_init_kernel, dim3(cm_grid(init_items)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  if (M > 0) {
    ursn_note_kernel("clmatch_entry");
    hipLaunchKernelGGL(clmatch_entry_kernel, dim3((unsigned)cdiv64(M, 256)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("clmatch_slot");
    hipLaunchKernelGGL(clmatch_slot_kernel, dim3(cm_grid(a.T)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("clmatch_row_a");
    hipLaunchKernelGGL(clmatch_row_kernel<0>, dim3(cm_grid(M)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("clmatch_row_b");
    hipLaunchKernelGGL(clmatch_row_kernel<1>, dim3(cm_grid(M)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
  }
  ursn_note_kernel("clmatch_event");
  hipLaunchKernelGGL(clmatch_event_kernel, dim3((unsigned)cdiv64(d->n, 256)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  if (out->pair_offsets) {
    ursn_note_kernel("clmatch_scan");
    hipLaunchKernelGGL(clmatch_scan_kernel, dim3(1), dim3(CM_SCAN_THREADS), 0, s, a);
    URSN_HIP(hipGetLastError());
    if (cells && M > 0 && out->pair_cap > 0) {
      ursn_note_kernel("clmatch_drop");
      hipLaunchKernelGGL(clmatch_drop_kernel, dim3(cm_grid(a.T)), dim3(256), 0, s, a);
      URSN_HIP(hipGetLastError());
      ursn_note_kernel("clmatch_rank");
      hipLaunchKernelGGL(clmatch_rank_kernel, dim3(cm_grid(M)), dim3(256), 0, s, a);
      URSN_HIP(hipGetLastError());
    }
  }
  return 0;
}
