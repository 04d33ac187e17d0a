// Cluster contact graph (gfx950): ursn_cluster_graph finds which clusters of ursn_cluster_voxels lie within `gap` voxels of each
// other (EDGES, with their near-pair counts and closest pair), reduces them to one record per row, joins the rows into interaction
// GROUPS (connected components of the edges) and reduces the entries to one record per group and per event.
// include/uresnet_hip.h names the columns; uresnet_amd/clusters.py (cluster_graph_numpy) states every field, and this file follows
// it: the same bits.  Every quantity is an integer; the one floating-point operation is the conversion of a value to its fixed-point
// charge (the object records' rule).
//
// Near pairs.  One thread per list entry with an id.  It visits the rows (d0, d1) of the volume that lie lexicographically before
// its own within +-gap, and the left part of its own row: (2 gap + 1) gap + gap + 1 = 5 / 13 / 25 rows in 3-D.  Each row costs one
// lower-bound binary search over [offsets[e], j) (at most 32 halvings) for the row's index interval clipped to the row, then at most
// 2 gap + 1 consecutive entries.  So every unordered pair of entries is seen once, from its higher list position; there is no dense
// map, and time and scratch follow the list.  Closeness is decided on coordinates: an interval never leaves its row, a row never
// leaves the volume, a search never leaves the event.
//
// Edges.  A near pair of two different rows adds to its edge in an open-addressing table in the scratch: 2^k >= 2 edge_cap + 2
// slots, the key (global row a << 32) | global row b, a < b, claimed with a 64-bit compare-and-swap from the EMPTY key the first
// launch writes; `pairs` and `touch` by 64-bit integer atomic adds; the closest pair by ONE packed 64-bit atomic minimum,
// dist2 << 40 | position in a << 9 | code of (x_b - x_a): inside one event and for one position in a, the position in b ascends
// with that code, so the minimum is the lexicographically smallest (dist2, pos_a, pos_b) whatever the arrival order.  The slot pass
// finds pos_b again with one binary search for index[pos_a] + the offset.  Claims are counted; more than edge_cap of them (or a
// probe walk that runs out, which needs a full table) set URSN_CLGRAPH_EDGE_OVERFLOW, and every later launch leaves at once: the
// count of distinct edges depends on the arguments alone.
//
// Contention.  Neighbouring entries mostly share their edge.  At every step of the (uniform) visiting loop the lanes of a wave that
// hold the same key next to each other are combined by a segmented shuffle reduction, the first lane of each run adds it to a
// 256-slot table of the workgroup in LDS, and the table is flushed once at the end: one global insertion per distinct edge of a
// workgroup.  A workgroup with more than 256 distinct edges finds the LDS table full (a probe walk capped at 256) and inserts the
// rest directly.  URSN_CLGRAPH_WAVE=0: one global insertion per near pair, the route the bits are compared against.
//
// Groups.  A pass over the occupied slots spreads each edge onto its two rows (degree, pairs, touching, the packed minimum
// dist2 << 32 | other row for `nearest`, the CSR count of the lower row) and links the rows in a union-find over global rows: 32-bit
// atomicMin to the lower root, walks through agent-scope relaxed loads that tolerate a stale word (an older link still names a true
// ancestor; the atomic's returned value decides), so a group's root is its lowest row whatever the order.  Then flatten, ONE
// workgroup scans the root flags and the CSR counts, one thread per row writes its record and adds to its group, one thread per
// entry writes its group and adds count, charge and box to it (wave runs and an LDS table first), one thread per group writes the
// record.  The edge list is scan / drop at an atomic cursor / rank by b inside the row's segment, like the match file's cells.
//
// Launches: init, near, slot, flatten, scan, row, entry, group; with an edge list: drop, rank.  Every loop is bounded.
#include "ursn_common.h"

#define CG_E URSN_CLGRAPH_E
#define CG_I URSN_CLGRAPH_I
#define CG_G URSN_CLGRAPH_G
#define CG_EV URSN_CLGRAPH_EV
enum { RW_DEG = 0, RW_PAIRS = 1, RW_TOUCH = 2, RW_NEAR = 3, RW_OUT = 4, RW_CURSOR = 5, RW = 6 };
enum { G_ROWS = 0, G_EDGES = 1, G_N = 2, G_CHARGE = 3, G_LO = 4, G_HI = 7, G_FIRST = 10, G_MASK = 11 };
enum { ST_IDS = 1, ST_EMPTY_ROW = 2, ST_INDEX = 4, ST_LOOP = 8, ST_CLASS = 16 };
#define CG_GRID_CAP 16384    // workgroup cap of the striding kernels
#define CG_SCAN_THREADS 1024
#define CG_BIG (1 << 20)     // above every coordinate

typedef long long cg_i64;
typedef unsigned long long cg_u64;
#define CG_EMPTY (~0ull)

struct CgArgs {
  ursn_cluster_graph_desc d;
  ursn_cluster_graph_out o;
  int32_t M;          // == d.m_total
  int32_t D0, D1, D2; // the volume as three extents (2-D: 1, s0, s1)
  int32_t g;          // gap
  int64_t V;          // D0 D1 D2
  int64_t T;          // slots, a power of two
  int shift;          // 64 - log2(T)
  int64_t edge_cap;
  cg_u64* key;        // [T]
  cg_i64* pairs;      // [T]
  cg_i64* touch;      // [T]
  cg_u64* best;       // [T] dist2 << 40 | pos_a << 9 | offset code
  int32_t* posb;      // [T]
  cg_i64* row;        // [max(M, 1)][RW]
  int32_t* parent;    // [max(M, 1)]
  int32_t* root;      // [max(M, 1)]
  int32_t* has;       // [max(M, 1)] 1: the row has a member
  int64_t* gscan;     // [max(M, 1) + 1] exclusive scan of the root flags = global group of a root
  int64_t* escan;     // [max(M, 1) + 1] exclusive scan of the rows' edge counts
  cg_i64* gacc;       // [max(M, 1)][CG_G] by global group
  int32_t* seg;       // [max(edge_cap, 1)] slot of each edge, by row a, unordered inside a row
  cg_i64* nclaim;     // [1] claimed slots = distinct edges
  int combine;
};

#define CG_LOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ void cg_add(cg_i64* p, cg_i64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cg_min(cg_i64* p, cg_i64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cg_max(cg_i64* p, cg_i64 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cg_or(cg_i64* p, cg_i64 v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cg_umin(cg_u64* p, cg_u64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cg_status(const CgArgs& a, int bits) {
  __hip_atomic_fetch_or(a.o.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows that can have a member: the device-read count, never more than the list could fill (the scratch holds M rows).
__device__ __forceinline__ int64_t cg_rows(const CgArgs& a) {
  const int64_t k = a.d.table_offsets[a.d.n];
  return k < 0 ? 0 : k > a.M ? a.M : k;
}
__device__ __forceinline__ int64_t cg_clamp(int64_t x, int64_t K) { return x < 0 ? 0 : x > K ? K : x; }
// more distinct edges than the caller allowed: only *status is defined, and every launch after the insertions leaves at once
__device__ __forceinline__ bool cg_overflowed(const CgArgs& a) { return *a.nclaim > a.edge_cap; }

// The largest e in [0, n) with off[e] <= x: n <= 65535, at most 16 halvings.
__device__ __forceinline__ int cg_search(const int64_t* off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  for (int s = 0; s < 17 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first position in [lo, hi) whose index is >= target (hi if none): at most 32 halvings.
__device__ __forceinline__ int cg_lower(const int32_t* index, int lo, int hi, int32_t target) {
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1);
    if (index[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t cg_slot(const CgArgs& a, cg_u64 key) { return (int64_t)((key * 0x9E3779B97F4A7C15ull) >> a.shift); }

// one edge's share -> the global table
__device__ __forceinline__ void cg_insert(const CgArgs& a, cg_u64 key, cg_i64 pairs, cg_i64 touch, cg_u64 best) {
  int64_t slot = cg_slot(a, key);
  for (int64_t probe = 0; probe < a.T; ++probe) {
    cg_u64 old = __hip_atomic_load(&a.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == CG_EMPTY) {
      cg_u64 expect = CG_EMPTY;
      __hip_atomic_compare_exchange_strong(&a.key[slot], &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (expect == CG_EMPTY) cg_add(a.nclaim, 1);   // this thread claimed the slot: one more distinct edge
      old = expect == CG_EMPTY ? key : expect;
    }
    if (old == key) {
      cg_add(&a.pairs[slot], pairs);
      if (touch) cg_add(&a.touch[slot], touch);
      cg_umin(&a.best[slot], best);
      return;
    }
    slot = (slot + 1) & (a.T - 1);
    // a long walk in a table that already holds more than edge_cap edges: the call has overflowed whatever this edge adds
    if ((probe & 63) == 63 && __hip_atomic_load(a.nclaim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > a.edge_cap) return;
  }
  cg_status(a, URSN_CLGRAPH_EDGE_OVERFLOW);   // every slot holds another edge: T > edge_cap distinct edges
}

// A run = consecutive lanes of the wave with the same key (`none` = no key).  Returns the lane one past the end of this lane's run
// and whether this lane is the run's first.  Without combining every active lane is its own run.
__device__ __forceinline__ int cg_run(cg_u64 key, cg_u64 none, int lane, int combine, bool& lead) {
  const bool act = key != none;
  if (!combine) {
    lead = act;
    return lane + 1;
  }
  const cg_u64 up = __shfl_up(key, 1, 64);
  const bool head = act && (lane == 0 || up != key);
  const cg_u64 mh = __ballot(head), ma = __ballot(act);
  const cg_u64 above = ~((2ull << lane) - 1ull);   // lanes above this one (lane 63: none)
  const cg_u64 nb = (mh | ~ma) & above;
  lead = head;
  return act ? (nb ? __ffsll((cg_i64)nb) - 1 : 64) : lane + 1;
}

// Segmented suffix reductions by doubling: after the step of distance d a lane holds its run's lanes [lane, min(lane + 2d, end)).
// Every lane of the wave calls them; `combine` is uniform.
__device__ __forceinline__ cg_i64 cg_seg_sum(cg_i64 v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const cg_i64 o = __shfl_down(v, d, 64);
      if (lane + d < end) v += o;
    }
  }
  return v;
}
__device__ __forceinline__ cg_u64 cg_seg_umin(cg_u64 v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const cg_u64 o = __shfl_down(v, d, 64);
      if (lane + d < end && o < v) v = o;
    }
  }
  return v;
}
__device__ __forceinline__ int cg_seg_min(int v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(v, d, 64);
      if (lane + d < end && o < v) v = o;
    }
  }
  return v;
}
__device__ __forceinline__ int cg_seg_max(int v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_down(v, d, 64);
      if (lane + d < end && o > v) v = o;
    }
  }
  return v;
}

// ---- union-find over global rows (cluster.hip's walk): parent[x] <= x, links only point lower -------------------------------------
__device__ __forceinline__ int cg_find(int32_t* parent, int x, int cap, const CgArgs& a) {
  for (int h = 0;; ++h) {
    const int p = CG_LOAD32(parent + x);
    if ((uint32_t)p >= (uint32_t)x) return x;
    x = p;
    if (h > cap) {
      cg_status(a, ST_LOOP);
      return -1;
    }
  }
}

__device__ __forceinline__ void cg_union(int32_t* parent, int x, int y, int cap, const CgArgs& a) {
  for (int trip = 0;; ++trip) {
    if (trip > cap) {
      cg_status(a, ST_LOOP);
      return;
    }
    x = cg_find(parent, x, cap, a);
    y = cg_find(parent, y, cap, a);
    if (x < 0 || y < 0 || x == y) return;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) return;   // hi was a root at that instant and now points at lo
    x = old, y = lo;         // hi had a parent already (old < hi): join that with lo
  }
}

// ---- launch 1: status, the empty table, the rows and groups below the device-read count, the event sums ----------------------------
__global__ __launch_bounds__(256) void clgraph_init_kernel(CgArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int n = a.d.n;
  if (t0 == 0) {
    const int64_t k = a.d.table_offsets[n];
    *a.o.status = (k < 0 || k > a.M || a.d.table_offsets[0] != 0 || a.d.offsets[0] != 0 || a.d.offsets[n] != a.M) ? ST_IDS : 0;
    *a.nclaim = 0;
  }
  for (int64_t t = t0; t < a.T; t += step) a.key[t] = CG_EMPTY, a.pairs[t] = 0, a.touch[t] = 0, a.best[t] = CG_EMPTY;
  const int64_t K = cg_rows(a);
  for (int64_t t = t0; t < K; t += step) {
    cg_i64* row = a.row + t * RW;
    row[RW_DEG] = row[RW_PAIRS] = row[RW_TOUCH] = row[RW_OUT] = row[RW_CURSOR] = 0;
    row[RW_NEAR] = (cg_i64)CG_EMPTY;
    a.parent[t] = (int32_t)t, a.root[t] = (int32_t)t, a.has[t] = 0;
    cg_i64* g = a.gacc + t * CG_G;
    g[G_ROWS] = g[G_EDGES] = g[G_N] = g[G_CHARGE] = g[G_FIRST] = g[G_MASK] = 0;
    g[G_LO] = g[G_LO + 1] = g[G_LO + 2] = CG_BIG;
    g[G_HI] = g[G_HI + 1] = g[G_HI + 2] = -1;
  }
  for (int64_t t = t0; t < (int64_t)n * CG_EV; t += step) a.o.event[t] = 0;
}

// An entry's event, global row and coordinates, or false: no id, or ids / offsets / an index that do not fit (bits to report).
struct CgEntry {
  int e, row, id, x0, x1, x2, lo;
  int64_t ke, tbase;
};
__device__ __forceinline__ bool cg_entry(const CgArgs& a, int j, int64_t K, CgEntry& t, int& bits) {
  const int32_t id = a.d.cluster[j];
  if (id == -1) return false;
  const int e = cg_search(a.d.offsets, a.d.n, j);
  const int64_t lo = a.d.offsets[e], tb = a.d.table_offsets[e], ke = a.d.table_offsets[e + 1] - tb;
  if (lo > j || j >= a.d.offsets[e + 1] || lo < 0 || id < 0 || id >= ke || tb < 0 || tb + id >= K) {
    bits |= ST_IDS;
    return false;
  }
  const int32_t idx = a.d.index[j];
  if (idx < 0 || idx >= a.V) {
    bits |= ST_INDEX;
    return false;
  }
  t.e = e, t.id = id, t.row = (int)(tb + id), t.lo = (int)lo, t.ke = ke, t.tbase = tb;
  const int plane = a.D1 * a.D2, rem = idx % plane;
  t.x0 = idx / plane, t.x1 = rem / a.D2, t.x2 = rem % a.D2;
  return true;
}

// ---- launch 2: one thread per list entry: its near pairs with earlier entries into the table -----------------------------------------
__global__ __launch_bounds__(256) void clgraph_near_kernel(CgArgs a) {
  __shared__ cg_u64 tkey[256], tbest[256];
  __shared__ cg_i64 tpairs[256], ttouch[256];
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, j = (int)j64;
  const int64_t K = cg_rows(a);
  CgEntry t;
  bool valid = false;
  if (j64 < a.M) {
    int bits = 0;
    valid = cg_entry(a, j, K, t, bits);
    if (bits) cg_status(a, bits);
    if (valid) a.has[t.row] = 1;
  }
  if (a.combine) {
    tkey[threadIdx.x] = CG_EMPTY, tbest[threadIdx.x] = CG_EMPTY, tpairs[threadIdx.x] = 0, ttouch[threadIdx.x] = 0;
    __syncthreads();
  }
  const int g = a.g;
  for (int d0 = -g; d0 <= 0; ++d0) {
    for (int d1 = -g; d1 <= (d0 == 0 ? 0 : g); ++d1) {   // uniform: every lane of the workgroup walks the same rows
      const bool own = d0 == 0 && d1 == 0;
      bool open = false;
      int at = 0;
      int32_t base = 0, zhi = -1;
      if (valid) {
        const int y0 = t.x0 + d0, y1 = t.x1 + d1;
        const int zlo = t.x2 - g < 0 ? 0 : t.x2 - g;
        zhi = own ? t.x2 - 1 : (t.x2 + g > a.D2 - 1 ? a.D2 - 1 : t.x2 + g);
        if (y0 >= 0 && y1 >= 0 && y1 < a.D1 && zlo <= zhi) {
          base = (y0 * a.D1 + y1) * a.D2;
          at = cg_lower(a.d.index, t.lo, j, base + zlo);
          open = true;
          zhi += base;   // the last index of the interval
          base += zlo;   // the first
        }
      }
      for (int s = 0; s <= 2 * g; ++s) {
        cg_u64 key = CG_EMPTY, best = CG_EMPTY;
        cg_i64 touch = 0;
        if (open) {
          const int k = at + s;
          const int32_t ik = k < j ? a.d.index[k] : -1;
          if (k >= j || ik > zhi || ik < base) {
            open = false;
          } else {
            const int32_t idk = a.d.cluster[k];
            if (idk >= 0 && idk < t.ke && idk != t.id) {
              const int dz = (ik - base) + ((t.x2 - g < 0 ? 0 : t.x2 - g) - t.x2);   // x2 of k minus x2 of j
              const int ad0 = -d0, ad1 = d1 < 0 ? -d1 : d1, adz = dz < 0 ? -dz : dz;
              const int cheb = ad0 > ad1 ? (ad0 > adz ? ad0 : adz) : (ad1 > adz ? ad1 : adz);
              const cg_u64 dist2 = (cg_u64)(d0 * d0 + d1 * d1 + dz * dz);
              const uint32_t rk = (uint32_t)(t.tbase + idk), rj = (uint32_t)t.row;
              touch = cheb == 1 ? 1 : 0;
              // pos_a and x_b - x_a: the entry of the LOWER row is a
              const bool jlow = rj < rk;
              const int c0 = jlow ? d0 : -d0, c1 = jlow ? d1 : -d1, c2 = jlow ? dz : -dz;
              const cg_u64 code = (cg_u64)(((c0 + 3) * 7 + (c1 + 3)) * 7 + (c2 + 3));
              key = jlow ? ((cg_u64)rj << 32) | rk : ((cg_u64)rk << 32) | rj;
              best = (dist2 << 40) | ((cg_u64)(uint32_t)(jlow ? j : k) << 9) | code;
            }
          }
        }
        if (!a.combine) {
          if (key != CG_EMPTY) cg_insert(a, key, 1, touch, best);
          continue;
        }
        if (__ballot(key != CG_EMPTY) == 0) continue;   // uniform per wave
        bool lead;
        const int end = cg_run(key, CG_EMPTY, lane, 1, lead);
        touch = cg_seg_sum(touch, lane, end, 1);
        best = cg_seg_umin(best, lane, end, 1);
        if (lead) {
          const cg_i64 pairs = end - lane;
          uint32_t slot = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 56);
          bool placed = false;
          for (int probe = 0; probe < 256 && !placed; ++probe) {
            const cg_u64 old = atomicCAS(&tkey[slot], CG_EMPTY, key);
            if (old == CG_EMPTY || old == key) placed = true;
            else slot = (slot + 1) & 255;
          }
          if (placed) {
            __hip_atomic_fetch_add(&tpairs[slot], pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (touch) __hip_atomic_fetch_add(&ttouch[slot], touch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(&tbest[slot], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {   // more than 256 distinct edges in this workgroup: the rest go to the global table directly
            cg_insert(a, key, pairs, touch, best);
          }
        }
      }
    }
  }
  if (!a.combine) return;
  __syncthreads();
  const cg_u64 k = tkey[threadIdx.x];
  if (k != CG_EMPTY) cg_insert(a, k, tpairs[threadIdx.x], ttouch[threadIdx.x], tbest[threadIdx.x]);
}

// ---- launch 3: one thread per slot: an occupied one spreads its edge onto its rows and links them --------------------------------------
__global__ __launch_bounds__(256) void clgraph_slot_kernel(CgArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cg_overflowed(a)) {
    if (t0 == 0) cg_status(a, URSN_CLGRAPH_EDGE_OVERFLOW);
    return;
  }
  const int64_t K = cg_rows(a);
  for (int64_t t = t0; t < a.T; t += step) {
    const cg_u64 key = a.key[t];
    if (key == CG_EMPTY) continue;
    const uint32_t ra = (uint32_t)(key >> 32), rb = (uint32_t)key;
    if (ra >= K || rb >= K || ra >= rb) { cg_status(a, ST_LOOP); continue; }   // cannot happen: keys are made of checked rows
    const cg_i64 pairs = a.pairs[t], touch = a.touch[t];
    const cg_u64 best = a.best[t], dist2 = best >> 40;
    const int pos_a = (int)((best >> 9) & 0x7FFFFFFFu), code = (int)(best & 511u);
    const int c0 = code / 49 - 3, c1 = (code / 7) % 7 - 3, c2 = code % 7 - 3;
    // the partner of pos_a: the entry of the same event whose index is index[pos_a] + the offset
    int pos_b = -1;
    if (pos_a < a.M) {
      const int e = cg_search(a.d.table_offsets, a.d.n, ra);
      int64_t lo = a.d.offsets[e], hi = a.d.offsets[e + 1];
      lo = cg_clamp(lo, a.M), hi = cg_clamp(hi, a.M);
      const int32_t target = a.d.index[pos_a] + (c0 * a.D1 + c1) * a.D2 + c2;
      const int p = cg_lower(a.d.index, (int)lo, (int)hi, target);
      if (p < hi && a.d.index[p] == target) pos_b = p;
    }
    if (pos_b < 0) cg_status(a, ST_LOOP);
    a.posb[t] = pos_b;
    cg_i64* wa = a.row + (int64_t)ra * RW;
    cg_i64* wb = a.row + (int64_t)rb * RW;
    cg_add(wa + RW_DEG, 1), cg_add(wb + RW_DEG, 1);
    cg_add(wa + RW_PAIRS, pairs), cg_add(wb + RW_PAIRS, pairs);
    if (touch > 0) cg_add(wa + RW_TOUCH, 1), cg_add(wb + RW_TOUCH, 1);
    cg_umin((cg_u64*)wa + RW_NEAR, (dist2 << 32) | rb);
    cg_umin((cg_u64*)wb + RW_NEAR, (dist2 << 32) | ra);
    cg_add(wa + RW_OUT, 1);
    cg_union(a.parent, (int)ra, (int)rb, (int)K, a);
  }
}

// ---- launch 4: one thread per row: its root ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clgraph_flatten_kernel(CgArgs a) {
  if (cg_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 256, K = cg_rows(a);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < K; r += step) {
    const int root = cg_find(a.parent, (int)r, (int)K, a);
    a.root[r] = root < 0 ? (int32_t)r : root;
  }
}

// ---- launch 5: one workgroup: exclusive scans of the root flags and of the rows' edge counts -------------------------------------------
__global__ __launch_bounds__(CG_SCAN_THREADS) void clgraph_scan_kernel(CgArgs a) {
  __shared__ cg_i64 pg[CG_SCAN_THREADS], pe[CG_SCAN_THREADS];
  if (cg_overflowed(a)) return;
  const int64_t K = cg_rows(a);
  const int64_t per = (K + CG_SCAN_THREADS - 1) / CG_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per < K ? (int64_t)threadIdx.x * per : K, hi = lo + per < K ? lo + per : K;
  cg_i64 sg = 0, se = 0;
  for (int64_t r = lo; r < hi; ++r) sg += a.root[r] == r ? 1 : 0, se += a.row[r * RW + RW_OUT];
  pg[threadIdx.x] = sg, pe[threadIdx.x] = se;
  __syncthreads();
  for (int d = 1; d < CG_SCAN_THREADS; d <<= 1) {   // inclusive scans of the chunk sums
    const cg_i64 og = (int)threadIdx.x >= d ? pg[threadIdx.x - d] : 0, oe = (int)threadIdx.x >= d ? pe[threadIdx.x - d] : 0;
    __syncthreads();
    pg[threadIdx.x] += og, pe[threadIdx.x] += oe;
    __syncthreads();
  }
  cg_i64 ag = pg[threadIdx.x] - sg, ae = pe[threadIdx.x] - se;
  for (int64_t r = lo; r < hi; ++r) {
    a.gscan[r] = ag, a.escan[r] = ae;
    if (a.o.edge_offsets && r <= a.o.cap_rows) a.o.edge_offsets[r] = ae;
    ag += a.root[r] == r ? 1 : 0, ae += a.row[r * RW + RW_OUT];
  }
  if (threadIdx.x == CG_SCAN_THREADS - 1) {
    a.gscan[K] = pg[threadIdx.x], a.escan[K] = pe[threadIdx.x];
    if (a.o.edge_offsets && K <= a.o.cap_rows) a.o.edge_offsets[K] = pe[threadIdx.x];
  }
}

// ---- launch 6: one thread per row: its record, its share of its group and of the event sums; the group offsets ---------------------------
__global__ __launch_bounds__(256) void clgraph_row_kernel(CgArgs a) {
  if (cg_overflowed(a)) return;
  const int lane = threadIdx.x & 63, n = a.d.n;
  const int64_t step = (int64_t)gridDim.x * 256, K = cg_rows(a);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e <= n; e += step) {
    const int64_t go = a.gscan[cg_clamp(a.d.table_offsets[e], K)];
    a.o.group_offsets[e] = go;
    if (e < n) a.o.event[e * CG_EV] = a.gscan[cg_clamp(a.d.table_offsets[e + 1], K)] - go;
  }
  for (int64_t base = (int64_t)blockIdx.x * 256; base < K; base += step) {   // uniform per workgroup: the shuffles need all lanes
    const int64_t r = base + threadIdx.x;
    int e = -1;
    cg_i64 out = 0, lonely = 0;
    if (r < K) {
      e = cg_search(a.d.table_offsets, n, r);
      const int64_t tb = a.d.table_offsets[e];
      if (tb > r || r >= a.d.table_offsets[e + 1]) {
        cg_status(a, ST_IDS), e = -1;          // table offsets that do not increase
      } else if (!a.has[r]) {
        cg_status(a, ST_EMPTY_ROW), e = -1;    // a row without members: not a table ursn_cluster_voxels wrote
      } else {
        const cg_i64* row = a.row + r * RW;
        const cg_i64 deg = row[RW_DEG];
        const cg_u64 near = (cg_u64)row[RW_NEAR];
        const int64_t root = a.root[r], g = a.gscan[root];
        out = row[RW_OUT], lonely = deg == 0 ? 1 : 0;
        if (r < a.o.cap_rows) {
          int64_t* t = a.o.rows + r * CG_I;
          t[0] = deg, t[1] = g - a.gscan[cg_clamp(tb, K)];
          t[2] = deg > 0 ? (int64_t)(uint32_t)near - tb : -1, t[3] = deg > 0 ? (int64_t)(near >> 32) : 0;
          t[4] = row[RW_PAIRS], t[5] = row[RW_TOUCH];
        }
        cg_i64* ga = a.gacc + g * CG_G;
        cg_add(ga + G_ROWS, 1);
        if (out) cg_add(ga + G_EDGES, out);
        if (root == r) ga[G_FIRST] = r - tb;   // the one thread of the group's lowest row; no other writes this word
        if (a.d.cls) {
          const int c = a.d.cls[r];
          if (c < 32) cg_or(ga + G_MASK, 1ll << c);
          else cg_status(a, ST_CLASS);
        }
      }
    }
    bool lead;
    const int end = cg_run((cg_u64)(cg_i64)e, (cg_u64)(cg_i64)-1, lane, a.combine, lead);
    out = cg_seg_sum(out, lane, end, a.combine), lonely = cg_seg_sum(lonely, lane, end, a.combine);
    if (lead && out) cg_add((cg_i64*)a.o.event + (int64_t)e * CG_EV + 1, out);
    if (lead && lonely) cg_add((cg_i64*)a.o.event + (int64_t)e * CG_EV + 2, lonely);
  }
}

// ---- launch 7: one thread per list entry: its group, and its share of the group's count, charge and box -------------------------------
__device__ __forceinline__ void cg_group_add(cg_i64* ga, cg_i64 n, cg_i64 q, cg_i64 bad, const int* lo, const int* hi) {
  cg_add(ga + G_N, n);
  if (q) cg_add(ga + G_CHARGE, q);
  if (bad) cg_or(ga + G_MASK, 1ll << 32);
#pragma unroll
  for (int k = 0; k < 3; ++k) cg_min(ga + G_LO + k, lo[k]), cg_max(ga + G_HI + k, hi[k]);
}

__global__ __launch_bounds__(256) void clgraph_entry_kernel(CgArgs a) {
  __shared__ int32_t tkey[256], tbad[256], tlo[3][256], thi[3][256];
  __shared__ cg_i64 tn[256], tq[256];
  if (cg_overflowed(a)) return;
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t K = cg_rows(a);
  int32_t g = -1;
  cg_i64 q = 0, bad = 0;
  int lo[3] = {CG_BIG, CG_BIG, CG_BIG}, hi[3] = {-1, -1, -1};
  if (j64 < a.M) {
    CgEntry t;
    int bits = 0;
    int32_t local = -1;
    if (cg_entry(a, (int)j64, K, t, bits)) {
      g = (int32_t)a.gscan[a.root[t.row]];
      local = (int32_t)(g - a.gscan[cg_clamp(t.tbase, K)]);
      lo[0] = hi[0] = t.x0, lo[1] = hi[1] = t.x1, lo[2] = hi[2] = t.x2;
      if (a.d.value) {
        const float v = a.d.value[j64];
        if (fabsf(v) < 32768.f) q = (cg_i64)rint((double)v * 65536.0);
        else bad = 1;                  // too large for the fixed point, infinite or NaN
      }
    }
    a.o.group[j64] = local;
  }
  if (!a.combine) {
    if (g >= 0) cg_group_add(a.gacc + (int64_t)g * CG_G, 1, q, bad, lo, hi);
    return;
  }
  bool lead;
  const int end = cg_run((cg_u64)(cg_i64)g, (cg_u64)(cg_i64)-1, lane, 1, lead);
  q = cg_seg_sum(q, lane, end, 1), bad = cg_seg_sum(bad, lane, end, 1);
#pragma unroll
  for (int k = 0; k < 3; ++k) lo[k] = cg_seg_min(lo[k], lane, end, 1), hi[k] = cg_seg_max(hi[k], lane, end, 1);
  tkey[threadIdx.x] = -1, tbad[threadIdx.x] = 0, tn[threadIdx.x] = 0, tq[threadIdx.x] = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) tlo[k][threadIdx.x] = CG_BIG, thi[k][threadIdx.x] = -1;
  __syncthreads();
  if (lead) {
    uint32_t slot = ((uint32_t)g * 2654435761u) >> 24;
    bool placed = false;
    for (int probe = 0; probe < 256 && !placed; ++probe) {
      const int32_t old = atomicCAS(&tkey[slot], -1, g);
      if (old == -1 || old == g) placed = true;
      else slot = (slot + 1) & 255;
    }
    if (placed) {
      __hip_atomic_fetch_add(&tn[slot], (cg_i64)(end - lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (q) __hip_atomic_fetch_add(&tq[slot], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (bad) __hip_atomic_fetch_or(&tbad[slot], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        __hip_atomic_fetch_min(&tlo[k][slot], lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&thi[k][slot], hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    } else {   // cannot happen (at most 256 runs, 256 slots); the totals still arrive
      cg_group_add(a.gacc + (int64_t)g * CG_G, end - lane, q, bad, lo, hi);
    }
  }
  __syncthreads();
  const int32_t k = tkey[threadIdx.x];
  if (k >= 0) {
    const int l[3] = {tlo[0][threadIdx.x], tlo[1][threadIdx.x], tlo[2][threadIdx.x]};
    const int h[3] = {thi[0][threadIdx.x], thi[1][threadIdx.x], thi[2][threadIdx.x]};
    cg_group_add(a.gacc + (int64_t)k * CG_G, tn[threadIdx.x], tq[threadIdx.x], tbad[threadIdx.x], l, h);
  }
}

// ---- launch 8: one thread per group: its record, and the event's largest group -----------------------------------------------------------
__global__ __launch_bounds__(256) void clgraph_group_kernel(CgArgs a) {
  if (cg_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 256, K = cg_rows(a);
  const int64_t G = a.gscan[K];
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < G && g < K; g += step) {
    const cg_i64* ga = a.gacc + g * CG_G;
    if (g < a.o.cap_groups) {
      int64_t* t = a.o.groups + g * CG_G;
      t[G_ROWS] = ga[G_ROWS], t[G_EDGES] = ga[G_EDGES], t[G_N] = ga[G_N], t[G_CHARGE] = ga[G_CHARGE];
      const int s = a.d.ndim == 2 ? 1 : 0;   // 2-D: the volume is (1, s0, s1) in here and x[2] = 0 outside
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const bool real = k + s < 3;
        t[G_LO + k] = real ? ga[G_LO + k + s] : 0, t[G_HI + k] = real ? ga[G_HI + k + s] : 0;
      }
      t[G_FIRST] = ga[G_FIRST], t[G_MASK] = ga[G_MASK];
    }
    const int e = cg_search(a.o.group_offsets, a.d.n, g);
    cg_max((cg_i64*)a.o.event + (int64_t)e * CG_EV + 3, ga[G_N]);
  }
}

// ---- launch 9: one thread per slot: an edge drops its slot into its row's segment ---------------------------------------------------------
__global__ __launch_bounds__(256) void clgraph_drop_kernel(CgArgs a) {
  if (cg_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 256, K = cg_rows(a);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < a.T; t += step) {
    const cg_u64 key = a.key[t];
    if (key == CG_EMPTY) continue;
    const uint32_t ra = (uint32_t)(key >> 32);
    if (ra >= K) continue;
    cg_i64* row = a.row + (int64_t)ra * RW;
    const cg_i64 pos = __hip_atomic_fetch_add(row + RW_CURSOR, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const cg_i64 at = a.escan[ra] + pos;
    if (pos < 0 || pos >= row[RW_OUT] || at < 0 || at >= a.edge_cap) cg_status(a, ST_LOOP);
    else a.seg[at] = (int32_t)t;       // T <= 2^31 slots
  }
}

// ---- launch 10: one thread per edge: its rank by b inside its segment, then the edge itself --------------------------------------------------
__global__ __launch_bounds__(256) void clgraph_rank_kernel(CgArgs a) {
  if (cg_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 256, K = cg_rows(a);
  int64_t total = a.escan[K];
  if (total > a.edge_cap) total = a.edge_cap;
  for (int64_t ci = (int64_t)blockIdx.x * 256 + threadIdx.x; ci < total; ci += step) {
    const int64_t t = (int64_t)(uint32_t)a.seg[ci];
    if (t >= a.T) { cg_status(a, ST_LOOP); continue; }
    const cg_u64 key = a.key[t];
    const uint32_t ra = (uint32_t)(key >> 32), rb = (uint32_t)key;
    if (key == CG_EMPTY || ra >= K) { cg_status(a, ST_LOOP); continue; }
    const int64_t s0 = a.escan[ra], cnt = a.row[(int64_t)ra * RW + RW_OUT];
    if (ci < s0 || ci >= s0 + cnt || s0 + cnt > a.edge_cap) { cg_status(a, ST_LOOP); continue; }
    int64_t rank = 0;
    for (int64_t k = 0; k < cnt; ++k) {   // bounded by the row's edges
      const int64_t u = (int64_t)(uint32_t)a.seg[s0 + k];
      if (u < a.T && (uint32_t)a.key[u] < rb) ++rank;
    }
    const int64_t at = s0 + rank;
    if (at < a.o.edge_out_cap) {
      const int e = cg_search(a.d.table_offsets, a.d.n, ra);
      const cg_u64 best = a.best[t];
      int64_t* o = a.o.edges + at * CG_E;
      o[0] = (int64_t)rb - a.d.table_offsets[e], o[1] = a.pairs[t], o[2] = a.touch[t], o[3] = (int64_t)(best >> 40);
      o[4] = (int64_t)((best >> 9) & 0x7FFFFFFFu), o[5] = a.posb[t];
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int64_t cg_slots(int64_t edge_cap) {
  int64_t t = 2;
  while (t < 2 * edge_cap + 2) t <<= 1;
  return t;
}

static size_t cg_layout(int64_t m_total, int64_t edge_cap, CgArgs* a, char* base) {
  const size_t T = (size_t)cg_slots(edge_cap), M1 = (size_t)(m_total < 1 ? 1 : m_total), E1 = (size_t)(edge_cap < 1 ? 1 : edge_cap);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 7) & ~(size_t)7; return p; };
  char* nclaim = take(8);
  char* key = take(T * 8);
  char* pairs = take(T * 8);
  char* touch = take(T * 8);
  char* best = take(T * 8);
  char* posb = take(T * 4);
  char* row = take(M1 * RW * 8);
  char* gacc = take(M1 * CG_G * 8);
  char* gscan = take((M1 + 1) * 8);
  char* escan = take((M1 + 1) * 8);
  char* parent = take(M1 * 4);
  char* root = take(M1 * 4);
  char* has = take(M1 * 4);
  char* seg = take(E1 * 4);
  if (a) {
    a->nclaim = (cg_i64*)nclaim, a->key = (cg_u64*)key, a->pairs = (cg_i64*)pairs, a->touch = (cg_i64*)touch, a->best = (cg_u64*)best;
    a->posb = (int32_t*)posb, a->row = (cg_i64*)row, a->gacc = (cg_i64*)gacc, a->gscan = (int64_t*)gscan, a->escan = (int64_t*)escan;
    a->parent = (int32_t*)parent, a->root = (int32_t*)root, a->has = (int32_t*)has, a->seg = (int32_t*)seg;
    a->T = (int64_t)T;
    int lg = 0;
    while (((size_t)1 << lg) < T) ++lg;
    a->shift = 64 - lg;
  }
  return off;
}

extern "C" size_t ursn_cluster_graph_scratch_bytes(int32_t n, int64_t m_total, int64_t cap_rows, int64_t cap_groups, int64_t edge_cap) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 31) || cap_rows < 0 || cap_groups < 0 || edge_cap < 0 ||
      edge_cap >= ((int64_t)1 << 30))
    return 0;
  return cg_layout(m_total, edge_cap, nullptr, nullptr);
}

static unsigned cg_grid(int64_t items) {
  const int64_t b = cdiv64(items, 256);
  return (unsigned)(b < 1 ? 1 : b > CG_GRID_CAP ? CG_GRID_CAP : b);
}

extern "C" int ursn_cluster_graph(const ursn_cluster_graph_desc* d, const ursn_cluster_graph_out* out, void* scratch,
                                  size_t scratch_bytes, void* stream) {
  const char* who = "cluster_graph";
  URSN_REQUIRE(d && out, "%s: null desc / out", who);
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)d->n);
  URSN_REQUIRE(d->m_total >= 0 && d->m_total < ((int64_t)1 << 31), "%s: m_total = %lld outside [0, 2^31)", who,
               (long long)d->m_total);
  URSN_REQUIRE(d->ndim == 2 || d->ndim == 3, "%s: ndim = %d, expected 2 or 3", who, (int)d->ndim);
  int64_t vol = 1;
  for (int k = 0; k < d->ndim; ++k) {
    URSN_REQUIRE(d->spatial[k] >= 1 && d->spatial[k] <= 32768, "%s: spatial[%d] = %d outside [1, 32768]", who, k, (int)d->spatial[k]);
    vol *= d->spatial[k];
  }
  URSN_REQUIRE(vol < ((int64_t)1 << 31), "%s: %lld voxels, expected fewer than 2^31", who, (long long)vol);
  URSN_REQUIRE(d->gap >= 1 && d->gap <= 3, "%s: gap = %d outside [1, 3]", who, (int)d->gap);
  URSN_REQUIRE(d->edge_cap >= 0 && d->edge_cap < ((int64_t)1 << 30), "%s: edge_cap = %lld outside [0, 2^30)", who,
               (long long)d->edge_cap);
  URSN_REQUIRE(out->cap_rows >= 0, "%s: cap_rows = %lld < 0", who, (long long)out->cap_rows);
  URSN_REQUIRE(out->cap_groups >= 0, "%s: cap_groups = %lld < 0", who, (long long)out->cap_groups);
  URSN_REQUIRE(out->edge_out_cap >= 0, "%s: edge_out_cap = %lld < 0", who, (long long)out->edge_out_cap);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster), "%s: null index / cluster", who);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->group_offsets && out->event, "%s: null out->group_offsets / out->event", who);
  URSN_REQUIRE(d->m_total == 0 || out->group, "%s: null out->group", who);
  URSN_REQUIRE(out->cap_rows == 0 || out->rows, "%s: null out->rows", who);
  URSN_REQUIRE(out->cap_groups == 0 || out->groups, "%s: null out->groups", who);
  URSN_REQUIRE(!out->edges || out->edge_offsets, "%s: out->edges needs out->edge_offsets", who);
  URSN_REQUIRE(out->edge_out_cap == 0 || !out->edge_offsets || out->edges, "%s: edge_out_cap = %lld with null out->edges", who,
               (long long)out->edge_out_cap);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)out->rows | (uintptr_t)out->groups |
                 (uintptr_t)out->group_offsets | (uintptr_t)out->event | (uintptr_t)out->edge_offsets | (uintptr_t)out->edges |
                 (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / rows / groups / group_offsets / event / edge_offsets / edges / scratch must be 8-byte "
               "aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->cluster | (uintptr_t)d->value | (uintptr_t)out->group | (uintptr_t)out->status) &
                3) == 0,
               "%s: index / cluster / value / group / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_graph_scratch_bytes(d->n, d->m_total, out->cap_rows, out->cap_groups, d->edge_cap);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  CgArgs a;
  a.d = *d;
  a.o = *out;
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.D0 = d->ndim == 3 ? d->spatial[0] : 1, a.D1 = d->spatial[d->ndim - 2], a.D2 = d->spatial[d->ndim - 1];
  a.V = vol, a.g = d->gap, a.edge_cap = d->edge_cap;
  cg_layout(M, d->edge_cap, &a, (char*)scratch);
  a.combine = ursn_env_on("URSN_CLGRAPH_WAVE") ? 1 : 0;   // read at every call: the two routes are compared in one process
  hipStream_t s = (hipStream_t)stream;
  ursn_note_kernel("clgraph_init");
  hipLaunchKernelGGL(clgraph_init_kernel, dim3(cg_grid(a.T > M ? a.T : M)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  if (M > 0) {
    ursn_note_kernel("clgraph_near");
    hipLaunchKernelGGL(clgraph_near_kernel, dim3((unsigned)cdiv64(M, 256)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("clgraph_slot");
    hipLaunchKernelGGL(clgraph_slot_kernel, dim3(cg_grid(a.T)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("clgraph_flatten");
    hipLaunchKernelGGL(clgraph_flatten_kernel, dim3(cg_grid(M)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
  }
  ursn_note_kernel("clgraph_scan");
  hipLaunchKernelGGL(clgraph_scan_kernel, dim3(1), dim3(CG_SCAN_THREADS), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clgraph_row");
  hipLaunchKernelGGL(clgraph_row_kernel, dim3(cg_grid(M > d->n ? M : d->n + 1)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  if (M > 0) {
    ursn_note_kernel("clgraph_entry");
    hipLaunchKernelGGL(clgraph_entry_kernel, dim3((unsigned)cdiv64(M, 256)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("clgraph_group");
    hipLaunchKernelGGL(clgraph_group_kernel, dim3(cg_grid(M)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    if (out->edges && out->edge_out_cap > 0 && d->edge_cap > 0) {
      ursn_note_kernel("clgraph_drop");
      hipLaunchKernelGGL(clgraph_drop_kernel, dim3(cg_grid(a.T)), dim3(256), 0, s, a);
      URSN_HIP(hipGetLastError());
      ursn_note_kernel("clgraph_rank");
      hipLaunchKernelGGL(clgraph_rank_kernel, dim3(cg_grid(d->edge_cap)), dim3(256), 0, s, a);
      URSN_HIP(hipGetLastError());
    }
  }
  return 0;
}
