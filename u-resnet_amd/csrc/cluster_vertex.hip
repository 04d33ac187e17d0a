// Vertex candidates (gfx950): ursn_cluster_vertices joins the end points of the object records (ursn_cluster_features) that lie
// within `radius` voxels of each other into VERTICES, counts per (vertex, cluster row) the entries of that row near the vertex's end
// points (INCIDENCES: the row's own ends, or its body passing by), and reduces them to one record per vertex, per row and per event.
// include/uresnet_hip.h names the columns; uresnet_amd/clusters.py (cluster_vertices_numpy) states every field operation by
// operation, and this file follows it: the same bits.
//
// Why the bits do not move.  Which end points are linked, and which entries are near an end point, is decided per pair on
// coordinates alone.  Vertices are the components of a union-find whose links only ever point at a lower key, so a root is its
// component's lowest key whatever the order of the unions, and a vertex's number is the count of roots before its own.  Everything
// accumulated across threads is a 64-bit INTEGER (atomic add / min / max / or at agent scope): exact in any order and grouping.
// Bounds with every extent <= 32768, m_total < 2^30 (so that every key 2 r + side is an int32) and K rows: near < 2 K * 343 < 2^41
// in an incidence, a vertex or summed; the incident rows of a vertex are distinct rows of one event, so n < 2^31 and
// |charge| <= 2^62; |s| < 2^15 * 2^32 = 2^47; the packed words: vertex << 32 | row (a vertex below 2 K < 2^31, a row below 2^30),
// dist2 << 32 | position (dist2 <= 27, a position below 2^30) and rows << 32 | n (rows below 2^30, n below 2^31, so the word is
// below 2^63 and orders as (rows, n)).  Every fp64 value is computed by ONE thread per vertex in the statement's order under
// contract(off); the end directions reach it in ascending key order because the incidence list it walks is ranked by row.  No
// float atomics.
//
// The neighbourhood walk.  From an end point, the (2 radius + 1)^2 rows (d0, d1) of the volume around it (a 2-D list runs as the
// volume (1, s0, s1)); per row ONE lower-bound binary search in the event's range for the row's index interval clipped to the row,
// then at most 2 radius + 1 consecutive entries.  No dense map.  There are few end points (at most 2 K) and up to 49 rows each, so
// the walk is built as one wave64 per end point with one lane per row (9 / 25 / 49 active lanes): the searches of one end point run
// side by side and touch neighbouring cache lines.  In the incidence pass the lanes of a wave that hold the same key next to each
// other are combined by a segmented shuffle reduction (runs by ballot), the first lane of each run adds it to a 256-slot table of the
// workgroup in LDS (open addressing, 64-bit integer LDS atomics), a run that finds the table full after 256 probes is inserted into
// the global table directly, and the LDS table is flushed once at the end.  URSN_CLVTX_WAVE=0 is the plain form: one thread per end
// point walks the rows one after another and makes one global insertion per pair; the same bits.
//
// Launches: (1) init: the status word (stored once; nothing in this launch ors into it), the empty table, per row its eligibility
// (parent = own key or -1), the bits that row has to report (a scratch word per row) and the cleared accumulators; (2) link: the
// walk, unions of end points of different rows; (3) flatten: the roots; it also ors the rows' bits into the status and checks EVERY
// entry with an id (its id inside its event's rows, its index inside the volume), whether or not a walk will meet it; (4) one
// workgroup scans the root flags: the vertex of a root and vertex_offsets' source; (5) ends: vertex_offsets, and count,
// coordinate sums and box of the end points per vertex;
// (6) incidence: the walk again, insertions keyed vertex << 32 | row; (7) slot: each incidence onto its vertex's accumulators, the
// overflow bit; (8) one workgroup scans the incidence counts into inc_offsets; (9) drop: event records cleared, row_vertex, each slot
// into its vertex's segment at an atomic cursor; (10) rank by row inside the segment, the incidence list; (11) one thread per vertex:
// its record, the cosines over at most 16 directions held in LDS, the event sums; (12) primary.  Every loop is bounded: an event
// search by 17 halvings, an index search by 32, a run of entries by 2 radius + 1, a probe walk by the slot count, a union-find walk
// by the key count, a rank and a direction walk by the vertex's incidences, the cosine loop by 16.
//
// The rank pass compares every incidence of a vertex with every other: cnt^2 reads for a vertex of cnt incidences.  That is small
// for what the call is for (tens of incidences per vertex), and quadratic for ids that are not objects: with min_size 1
// on a dense list of one-voxel clusters a single vertex can hold 10^5 and more incidences, and the launch then runs for minutes.
// The caller bounds it: inc_cap bounds the incidences of any vertex, and nothing is ranked after an overflow.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define VX_FI URSN_CLFEAT_I
#define VX_FR URSN_CLFEAT_R
#define VX_VI URSN_CLVTX_VI
#define VX_VR URSN_CLVTX_VR
#define VX_IN URSN_CLVTX_IN
#define VX_EV URSN_CLVTX_EV
enum { FI_N = 0, FI_CHARGE = 1, FI_END_LO = 24, FI_END_HI = 25, FR_AXIS = 12, FR_LEN = 15 };   // the object record's columns read here
enum { A_ENDS = 0, A_ROWS = 1, A_BODIES = 2, A_NEAR = 3, A_N = 4, A_CHARGE = 5, A_S = 6, A_LO = 9, A_HI = 12, A_MASK = 15, A_CURSOR = 16,
       VA = 17 };
enum { ST_IDS = 1, ST_EMPTY_ROW = 2, ST_INDEX = 4, ST_LOOP = 8, ST_CLASS = 16, ST_END = 32, ST_TABLE = 64 };
#define VX_GRID_CAP 4096       // workgroup cap of the striding kernels
#define VX_WAVE_GRID_CAP 1024  // workgroup cap of the two walk kernels: 4 end points per workgroup and sweep in the wave form
#define VX_SCAN_THREADS 1024
#define VX_DIRS 16             // end directions the cosines use
#define VX_BIG (1 << 20)       // above every coordinate

typedef long long vx_i64;
typedef unsigned long long vx_u64;
#define VX_EMPTY (~0ull)

struct VxArgs {
  ursn_cluster_vtx_desc d;
  ursn_cluster_vtx_out o;
  int32_t M;          // == d.m_total
  int32_t D0, D1, D2; // the volume as three extents (2-D: 1, s0, s1)
  int32_t g;          // radius
  int64_t V;          // D0 D1 D2
  int64_t Kmax;       // min(m_total, feat_cap): no more rows are considered
  int64_t T;          // slots, a power of two
  int shift;          // 64 - log2(T)
  int64_t inc_cap;
  vx_i64* nclaim;     // [1] claimed slots = distinct incidences
  vx_u64* key;        // [T] vertex << 32 | global row
  vx_i64* near;       // [T]
  vx_i64* kind;       // [T]
  vx_u64* best;       // [T] dist2 << 32 | position
  vx_i64* vacc;       // [2 M1][VA] by global vertex
  int64_t* iscan;     // [2 M1 + 1] exclusive scan of the vertices' incidence counts
  vx_i64* evmax;      // [n] rows << 32 | n of the event's primary vertex
  int32_t* parent;    // [2 M1] by key; -1: not an end point
  int32_t* root;      // [2 M1]
  int32_t* vnum;      // [2 M1 + 1] roots before the key = the global vertex of a root
  int32_t* vkey;      // [2 M1] the root key of a global vertex
  int32_t* seg;       // [max(inc_cap, 1)] slot of each incidence, by vertex, unordered inside a vertex
  int32_t* sorted;    // [max(inc_cap, 1)] the same, ascending by row inside a vertex
  int32_t* rbits;     // [M1] status bits launch 1 found at a row; launch 3 reports them
  int combine;
};

#define VX_LOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ void vx_add(vx_i64* p, vx_i64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_min(vx_i64* p, vx_i64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_max(vx_i64* p, vx_i64 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_or(vx_i64* p, vx_i64 v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_umin(vx_u64* p, vx_u64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void vx_status(const VxArgs& a, int bits) {
  __hip_atomic_fetch_or(a.o.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows considered: the device-read count, never more than the list could fill or the object tables hold.
__device__ __forceinline__ int64_t vx_rows(const VxArgs& a) {
  const int64_t k = a.d.table_offsets[a.d.n];
  return k < 0 ? 0 : k > a.Kmax ? a.Kmax : k;
}
__device__ __forceinline__ int64_t vx_clamp(int64_t x, int64_t K) { return x < 0 ? 0 : x > K ? K : x; }
// more distinct incidences than the caller allowed: the launches after the insertions leave at once
__device__ __forceinline__ bool vx_overflowed(const VxArgs& a) { return *a.nclaim > a.inc_cap; }

// The largest e in [0, n) with off[e] <= x: n <= 65535, at most 16 halvings.
__device__ __forceinline__ int vx_search(const int64_t* off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  for (int s = 0; s < 17 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first position in [lo, hi) whose index is >= target (hi if none): at most 32 halvings.
__device__ __forceinline__ int vx_lower(const int32_t* index, int lo, int hi, int32_t target) {
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1);
    if (index[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t vx_slot(const VxArgs& a, vx_u64 key) { return (int64_t)((key * 0x9E3779B97F4A7C15ull) >> a.shift); }

// one incidence's share -> the global table
__device__ __forceinline__ void vx_insert(const VxArgs& a, vx_u64 key, vx_i64 near, vx_i64 kind, vx_u64 best) {
  int64_t slot = vx_slot(a, key);
  for (int64_t probe = 0; probe < a.T; ++probe) {
    vx_u64 old = __hip_atomic_load(&a.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == VX_EMPTY) {
      vx_u64 expect = VX_EMPTY;
      __hip_atomic_compare_exchange_strong(&a.key[slot], &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (expect == VX_EMPTY) vx_add(a.nclaim, 1);   // this thread claimed the slot: one more distinct incidence
      old = expect == VX_EMPTY ? key : expect;
    }
    if (old == key) {
      vx_add(&a.near[slot], near);
      if (kind) vx_or(&a.kind[slot], kind);
      vx_umin(&a.best[slot], best);
      return;
    }
    slot = (slot + 1) & (a.T - 1);
    // a long walk in a table that already holds more than inc_cap incidences: the call has overflowed whatever this one adds
    if ((probe & 63) == 63 && __hip_atomic_load(a.nclaim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > a.inc_cap) return;
  }
  vx_status(a, URSN_CLVTX_INC_OVERFLOW);   // every slot holds another incidence: T > inc_cap distinct ones
}

// A run = consecutive lanes of the wave with the same key.  Returns the lane one past the end of this lane's run and whether this
// lane is the run's first.  Every lane of the wave calls it.
__device__ __forceinline__ int vx_run(vx_u64 key, int lane, bool& lead) {
  const bool act = key != VX_EMPTY;
  const vx_u64 up = __shfl_up(key, 1, 64);
  const bool head = act && (lane == 0 || up != key);
  const vx_u64 mh = __ballot(head), ma = __ballot(act);
  const vx_u64 above = ~((2ull << lane) - 1ull);   // lanes above this one (lane 63: none)
  const vx_u64 nb = (mh | ~ma) & above;
  lead = head;
  return act ? (nb ? __ffsll((vx_i64)nb) - 1 : 64) : lane + 1;
}
// Segmented suffix reductions by doubling: after the step of distance d a lane holds its run's lanes [lane, min(lane + 2d, end)).
__device__ __forceinline__ int vx_seg_or(int v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_down(v, d, 64);
    if (lane + d < end) v |= o;
  }
  return v;
}
__device__ __forceinline__ vx_u64 vx_seg_umin(vx_u64 v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const vx_u64 o = __shfl_down(v, d, 64);
    if (lane + d < end && o < v) v = o;
  }
  return v;
}

// ---- union-find over keys (cluster.hip's walk): parent[x] <= x, links only point lower ------------------------------------------------
__device__ __forceinline__ int vx_find(int32_t* parent, int x, int cap, const VxArgs& a) {
  for (int h = 0;; ++h) {
    const int p = VX_LOAD32(parent + x);
    if ((uint32_t)p >= (uint32_t)x) return x;   // a root (p == x), or no end point (p == -1)
    x = p;
    if (h > cap) {
      vx_status(a, ST_LOOP);
      return -1;
    }
  }
}

__device__ __forceinline__ void vx_union(int32_t* parent, int x, int y, int cap, const VxArgs& a) {
  for (int trip = 0;; ++trip) {
    if (trip > cap) {
      vx_status(a, ST_LOOP);
      return;
    }
    x = vx_find(parent, x, cap, a);
    y = vx_find(parent, y, cap, a);
    if (x < 0 || y < 0 || x == y) return;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) return;   // hi was a root at that instant and now points at lo
    x = old, y = lo;         // hi had a parent already (old < hi): join that with lo
  }
}

// An end point: its key's row and event, the event's list range, its position and coordinates.  Only keys that launch 1 accepted
// (parent != -1) come here: their event, position and index were checked there.
struct VxEnd {
  int row, id, lo, hi, pos, x0, x1, x2;
  int64_t ke, tbase;
};
__device__ __forceinline__ void vx_end(const VxArgs& a, int key, VxEnd& t) {
  const int r = key >> 1;
  const int e = vx_search(a.d.table_offsets, a.d.n, r);
  t.row = r, t.tbase = a.d.table_offsets[e], t.ke = a.d.table_offsets[e + 1] - t.tbase, t.id = (int)(r - t.tbase);
  t.lo = (int)vx_clamp(a.d.offsets[e], a.M), t.hi = (int)vx_clamp(a.d.offsets[e + 1], a.M);
  t.pos = (int)a.d.itab[(int64_t)r * VX_FI + FI_END_LO + (key & 1)];
  const int32_t idx = a.d.index[t.pos];
  const int plane = a.D1 * a.D2, rem = idx % plane;
  t.x0 = idx / plane, t.x1 = rem / a.D2, t.x2 = rem % a.D2;
}

// One row (d0, d1) of the volume around an end point: the list range [at, ...) of its entries within +-g of x2; false: no such row.
struct VxRow {
  int at;
  int32_t first, last;   // the index interval
};
__device__ __forceinline__ bool vx_row(const VxArgs& a, const VxEnd& t, int d0, int d1, VxRow& w) {
  const int y0 = t.x0 + d0, y1 = t.x1 + d1;
  if (y0 < 0 || y0 >= a.D0 || y1 < 0 || y1 >= a.D1) return false;
  const int zlo = t.x2 - a.g < 0 ? 0 : t.x2 - a.g, zhi = t.x2 + a.g > a.D2 - 1 ? a.D2 - 1 : t.x2 + a.g;
  const int32_t base = (y0 * a.D1 + y1) * a.D2;
  w.first = base + zlo, w.last = base + zhi;
  w.at = vx_lower(a.d.index, t.lo, t.hi, w.first);
  return true;
}

// ---- launch 1: status, the empty table, per row its eligibility and the cleared accumulators ------------------------------------------
__global__ __launch_bounds__(256) void clvtx_init_kernel(VxArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int n = a.d.n;
  if (t0 == 0) {
    const int64_t k = a.d.table_offsets[n];
    int bits = (k < 0 || k > a.M || a.d.table_offsets[0] != 0 || a.d.offsets[0] != 0 || a.d.offsets[n] != a.M) ? ST_IDS : 0;
    if (k > a.d.feat_cap) bits |= ST_TABLE;
    *a.o.status = bits;
    *a.nclaim = 0;
  }
  for (int64_t t = t0; t < a.T; t += step) a.key[t] = VX_EMPTY, a.near[t] = 0, a.kind[t] = 0, a.best[t] = VX_EMPTY;
  for (int64_t t = t0; t < n; t += step) a.evmax[t] = 0;
  const int64_t K = vx_rows(a);
  for (int64_t r = t0; r < K; r += step) {
    const int64_t* it = a.d.itab + r * VX_FI;
    const int64_t cnt = it[FI_N], elo = it[FI_END_LO], ehi = it[FI_END_HI];
    const int e = vx_search(a.d.table_offsets, n, r);
    const int64_t tb = a.d.table_offsets[e];
    int bits = 0;
    bool ok = true;
    if (tb > r || r >= a.d.table_offsets[e + 1]) bits |= ST_IDS, ok = false;   // table offsets that do not increase
    else if (cnt <= 0) bits |= ST_EMPTY_ROW, ok = false;                         // not a row ursn_cluster_features wrote
    if (ok && a.d.cls && a.d.cls[r] >= 32) bits |= ST_CLASS, ok = false;
    if (ok && (cnt < a.d.min_size || (a.d.class_mask && !((a.d.class_mask >> a.d.cls[r]) & 1u)))) ok = false;
    if (ok) {
      const int64_t lo = vx_clamp(a.d.offsets[e], a.M), hi = vx_clamp(a.d.offsets[e + 1], a.M);
      for (int side = 0; side < 2 && ok; ++side) {
        const int64_t p = side ? ehi : elo;
        if (p < lo || p >= hi || a.d.cluster[p] != r - tb) bits |= ST_END, ok = false;
        else if (a.d.index[p] < 0 || a.d.index[p] >= a.V) bits |= ST_INDEX, ok = false;
      }
    }
    a.rbits[r] = bits;   // reported by launch 3: an or in this launch could land before thread 0's store and be erased
    a.parent[2 * r] = ok ? (int32_t)(2 * r) : -1;
    a.parent[2 * r + 1] = ok && ehi != elo ? (int32_t)(2 * r + 1) : -1;
    for (int side = 0; side < 2; ++side) {
      vx_i64* v = a.vacc + (2 * r + side) * VA;
      for (int c = 0; c < VA; ++c) v[c] = 0;
      v[A_LO] = v[A_LO + 1] = v[A_LO + 2] = VX_BIG;
      v[A_HI] = v[A_HI + 1] = v[A_HI + 2] = -1;
    }
  }
}

// The keys of the two walk kernels.  WAVE: a workgroup takes 4 keys per sweep, one per wave; else 256, one per thread.
template <bool WAVE>
__device__ __forceinline__ int64_t vx_first_key() { return WAVE ? (int64_t)blockIdx.x * 4 : (int64_t)blockIdx.x * 256; }
template <bool WAVE>
__device__ __forceinline__ int64_t vx_key_step() { return (int64_t)gridDim.x * (WAVE ? 4 : 256); }

// ---- launch 2: the walk from every end point: an end point of another row in reach is linked --------------------------------------------
__device__ __forceinline__ void vx_link_row(const VxArgs& a, const VxEnd& t, int key, int d0, int d1, int64_t K) {
  VxRow w;
  if (!vx_row(a, t, d0, d1, w)) return;
  for (int s = 0; s <= 2 * a.g; ++s) {
    const int k = w.at + s;
    if (k >= t.hi) return;
    const int32_t ik = a.d.index[k];
    if (ik > w.last || ik < w.first) return;
    const int32_t idk = a.d.cluster[k];
    if (idk < 0 || idk >= t.ke) {
      if (idk != -1) vx_status(a, ST_IDS);
      continue;
    }
    const int64_t rk = t.tbase + idk;
    if (rk >= K || rk == t.row || VX_LOAD32(a.parent + 2 * rk) == -1) continue;   // beyond the rows, its own row, or not eligible
    const int64_t* it = a.d.itab + rk * VX_FI;
    const int other = k == it[FI_END_LO] ? (int)(2 * rk) : k == it[FI_END_HI] ? (int)(2 * rk + 1) : -1;
    if (other >= 0 && other < key) vx_union(a.parent, key, other, (int)(2 * K), a);   // every link is seen from both ends
  }
}

template <bool WAVE>
__global__ __launch_bounds__(256) void clvtx_link_kernel(VxArgs a) {
  const int64_t K = vx_rows(a), keys = 2 * K;
  const int lane = threadIdx.x & 63, w = 2 * a.g + 1;
  for (int64_t base = vx_first_key<WAVE>(); base < keys; base += vx_key_step<WAVE>()) {
    const int64_t key = base + (WAVE ? threadIdx.x >> 6 : threadIdx.x);
    if (key >= keys || VX_LOAD32(a.parent + key) == -1) continue;
    VxEnd t;
    vx_end(a, (int)key, t);
    if (WAVE) {
      if (lane < w * w) vx_link_row(a, t, (int)key, lane / w - a.g, lane % w - a.g, K);
    } else {
      for (int d0 = -a.g; d0 <= a.g; ++d0)
        for (int d1 = -a.g; d1 <= a.g; ++d1) vx_link_row(a, t, (int)key, d0, d1, K);
    }
  }
}

// ---- launch 3: one thread per key: its root; the bits launch 1 left for its row; one thread per entry: is it consistent ----------------
__global__ __launch_bounds__(256) void clvtx_flatten_kernel(VxArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = vx_rows(a), keys = 2 * K;
  for (int64_t k = t0; k < keys; k += step) {
    a.root[k] = a.parent[k] == -1 ? -1 : vx_find(a.parent, (int)k, (int)keys, a);   // a walk that ran out: -1, no end point
    if (!(k & 1) && a.rbits[k >> 1]) vx_status(a, a.rbits[k >> 1]);
  }
  for (int64_t j = t0; j < a.M; j += step) {   // every entry with an id, as the statement checks it; the walks skip what fails here
    const int32_t id = a.d.cluster[j];
    if (id == -1) continue;
    const int e = vx_search(a.d.offsets, a.d.n, j);
    int bits = 0;
    if (a.d.offsets[e] > j || j >= a.d.offsets[e + 1] || id < 0 || id >= a.d.table_offsets[e + 1] - a.d.table_offsets[e]) bits |= ST_IDS;
    if (a.d.index[j] < 0 || a.d.index[j] >= a.V) bits |= ST_INDEX;
    if (bits) vx_status(a, bits);
  }
}

// ---- launches 4 and 8: one workgroup: an exclusive scan, a chunk per thread --------------------------------------------------------------
// mode 0: the root flags of the keys -> vnum, vkey.  mode 1: the incidence counts of the vertices -> iscan, inc_offsets.
__global__ __launch_bounds__(VX_SCAN_THREADS) void clvtx_scan_kernel(VxArgs a, int mode) {
  __shared__ vx_i64 part[VX_SCAN_THREADS];
  if (mode == 1 && vx_overflowed(a)) return;
  const int64_t keys = 2 * vx_rows(a);
  const int64_t N = mode == 0 ? keys : (int64_t)a.vnum[keys];
  const int64_t per = (N + VX_SCAN_THREADS - 1) / VX_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per < N ? (int64_t)threadIdx.x * per : N, hi = lo + per < N ? lo + per : N;
  vx_i64 sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += mode == 0 ? (a.root[i] == i ? 1 : 0) : a.vacc[i * VA + A_ROWS];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < VX_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunk sums
    const vx_i64 o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += o;
    __syncthreads();
  }
  vx_i64 at = part[threadIdx.x] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    if (mode == 0) {
      a.vnum[i] = (int32_t)at;
      if (a.root[i] == i) a.vkey[at] = (int32_t)i, ++at;
    } else {
      a.iscan[i] = at;
      if (i <= a.o.cap_vertices) a.o.inc_offsets[i] = at;
      at += a.vacc[i * VA + A_ROWS];
    }
  }
  if (threadIdx.x == VX_SCAN_THREADS - 1) {
    const vx_i64 total = part[threadIdx.x];
    if (mode == 0) {
      a.vnum[N] = (int32_t)total;
    } else {
      a.iscan[N] = total;
      if (N <= a.o.cap_vertices) a.o.inc_offsets[N] = total;
    }
  }
}

// The global vertex of a key, -1 for none.
__device__ __forceinline__ int64_t vx_vertex(const VxArgs& a, int64_t key) {
  const int32_t root = a.root[key];
  return root < 0 ? -1 : (int64_t)a.vnum[root];
}

// ---- launch 5: vertex_offsets; one thread per key: its end point into its vertex's count, coordinate sums and box ------------------------
__global__ __launch_bounds__(256) void clvtx_ends_kernel(VxArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = vx_rows(a), keys = 2 * K;
  for (int64_t e = t0; e <= a.d.n; e += step) a.o.vertex_offsets[e] = a.vnum[2 * vx_clamp(a.d.table_offsets[e], K)];
  for (int64_t key = t0; key < keys; key += step) {
    const int64_t v = vx_vertex(a, key);
    if (v < 0) continue;
    VxEnd t;
    vx_end(a, (int)key, t);
    vx_i64* acc = a.vacc + v * VA;
    const int x[3] = {t.x0, t.x1, t.x2};
    vx_add(acc + A_ENDS, 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (x[c]) vx_add(acc + A_S + c, x[c]);
      vx_min(acc + A_LO + c, x[c]), vx_max(acc + A_HI + c, x[c]);
    }
  }
}

// ---- launch 6: the walk again: every entry with an id in reach of an end point counts towards (the end point's vertex, its row) -------
__device__ __forceinline__ vx_u64 vx_pair(const VxArgs& a, const VxEnd& t, const VxRow& w, bool& open, int s, int d0, int d1, int side,
                                           vx_u64 vertex, int64_t K, int& kind, vx_u64& best) {
  const int k = w.at + s;
  if (k >= t.hi) {
    open = false;
    return VX_EMPTY;
  }
  const int32_t ik = a.d.index[k];
  if (ik > w.last || ik < w.first) {
    open = false;
    return VX_EMPTY;
  }
  const int32_t idk = a.d.cluster[k];
  if (idk < 0 || idk >= t.ke) {
    if (idk != -1) vx_status(a, ST_IDS);
    return VX_EMPTY;
  }
  const int64_t rk = t.tbase + idk;
  if (rk >= K) return VX_EMPTY;
  const int dz = ik % a.D2 - t.x2;
  kind = k == t.pos ? 1 << side : 0;
  best = ((vx_u64)(d0 * d0 + d1 * d1 + dz * dz) << 32) | (vx_u64)(uint32_t)k;
  return (vertex << 32) | (vx_u64)rk;
}

template <bool WAVE>
__global__ __launch_bounds__(256) void clvtx_incidence_kernel(VxArgs a) {
  __shared__ vx_u64 tkey[256], tbest[256];
  __shared__ vx_i64 tnear[256];
  __shared__ int tkind[256];
  const int64_t K = vx_rows(a), keys = 2 * K;
  const int lane = threadIdx.x & 63, w = 2 * a.g + 1;
  if (WAVE) {
    tkey[threadIdx.x] = VX_EMPTY, tbest[threadIdx.x] = VX_EMPTY, tnear[threadIdx.x] = 0, tkind[threadIdx.x] = 0;
    __syncthreads();
  }
  for (int64_t base = vx_first_key<WAVE>(); base < keys; base += vx_key_step<WAVE>()) {   // uniform per workgroup
    const int64_t key = base + (WAVE ? threadIdx.x >> 6 : threadIdx.x);
    const int64_t v = key < keys ? vx_vertex(a, key) : -1;
    if (v < 0) continue;                                   // uniform per wave in the wave form
    VxEnd t;
    vx_end(a, (int)key, t);
    const int side = (int)(key & 1);
    if (!WAVE) {
      for (int d0 = -a.g; d0 <= a.g; ++d0)
        for (int d1 = -a.g; d1 <= a.g; ++d1) {
          VxRow r;
          bool open = vx_row(a, t, d0, d1, r);
          for (int s = 0; s <= 2 * a.g && open; ++s) {
            int kind = 0;
            vx_u64 best = VX_EMPTY;
            const vx_u64 k64 = vx_pair(a, t, r, open, s, d0, d1, side, (vx_u64)v, K, kind, best);
            if (k64 != VX_EMPTY) vx_insert(a, k64, 1, kind, best);
          }
        }
      continue;
    }
    const int d0 = lane / w - a.g, d1 = lane % w - a.g;
    VxRow r;
    bool open = lane < w * w && vx_row(a, t, d0, d1, r);
    for (int s = 0; s <= 2 * a.g; ++s) {                   // uniform: every lane of the wave takes every step
      int kind = 0;
      vx_u64 best = VX_EMPTY, k64 = VX_EMPTY;
      if (open) k64 = vx_pair(a, t, r, open, s, d0, d1, side, (vx_u64)v, K, kind, best);
      if (__ballot(k64 != VX_EMPTY) == 0) continue;        // uniform per wave
      bool lead;
      const int end = vx_run(k64, lane, lead);
      kind = vx_seg_or(kind, lane, end);
      best = vx_seg_umin(best, lane, end);
      if (lead) {
        const vx_i64 near = end - lane;
        uint32_t slot = (uint32_t)((k64 * 0x9E3779B97F4A7C15ull) >> 56);
        bool placed = false;
        for (int probe = 0; probe < 256 && !placed; ++probe) {
          const vx_u64 old = atomicCAS(&tkey[slot], VX_EMPTY, k64);
          if (old == VX_EMPTY || old == k64) placed = true;
          else slot = (slot + 1) & 255;
        }
        if (placed) {
          __hip_atomic_fetch_add(&tnear[slot], near, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (kind) __hip_atomic_fetch_or(&tkind[slot], kind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_min(&tbest[slot], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {   // more than 256 distinct incidences in this workgroup: the rest go to the global table directly
          vx_insert(a, k64, near, kind, best);
        }
      }
    }
  }
  if (!WAVE) return;
  __syncthreads();
  const vx_u64 k = tkey[threadIdx.x];
  if (k != VX_EMPTY) vx_insert(a, k, tnear[threadIdx.x], tkind[threadIdx.x], tbest[threadIdx.x]);
}

// ---- launch 7: one thread per slot: an occupied one spreads its incidence onto its vertex; the overflow bit --------------------------------
__global__ __launch_bounds__(256) void clvtx_slot_kernel(VxArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vx_overflowed(a)) {
    if (t0 == 0) vx_status(a, URSN_CLVTX_INC_OVERFLOW);
    return;
  }
  const int64_t K = vx_rows(a), V = a.vnum[2 * K];
  for (int64_t t = t0; t < a.T; t += step) {
    const vx_u64 key = a.key[t];
    if (key == VX_EMPTY) continue;
    const int64_t v = (int64_t)(key >> 32), r = (int64_t)(uint32_t)key;
    if (v >= V || r >= K) { vx_status(a, ST_LOOP); continue; }   // cannot happen: keys are made of checked vertices and rows
    vx_i64* acc = a.vacc + v * VA;
    const int64_t* it = a.d.itab + r * VX_FI;
    vx_add(acc + A_ROWS, 1);
    if (a.kind[t] == 0) vx_add(acc + A_BODIES, 1);
    vx_add(acc + A_NEAR, a.near[t]);
    vx_add(acc + A_N, it[FI_N]);
    if (it[FI_CHARGE]) vx_add(acc + A_CHARGE, it[FI_CHARGE]);
    vx_i64 mask = a.d.rtab[r * VX_FR + FR_LEN] == 0.0 ? 2ll << 32 : 0;
    if (a.d.cls) {
      const int c = a.d.cls[r];
      if (c < 32) mask |= 1ll << c;
      else vx_status(a, ST_CLASS);
    }
    if (mask) vx_or(acc + A_MASK, mask);
  }
}

// ---- launch 9: the event records' start, row_vertex, and each incidence's slot into its vertex's segment ----------------------------------
__global__ __launch_bounds__(256) void clvtx_drop_kernel(VxArgs a) {
  if (vx_overflowed(a)) return;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = vx_rows(a), V = a.vnum[2 * K];
  for (int64_t e = t0; e < a.d.n; e += step) {
    const int64_t cnt = a.o.vertex_offsets[e + 1] - a.o.vertex_offsets[e];
    int64_t* ev = a.o.event + e * VX_EV;
    ev[0] = cnt, ev[1] = 0, ev[2] = 0, ev[3] = cnt > 0 ? INT64_MAX : -1;   // launch 12 lowers [3] to the primary vertex
  }
  for (int64_t r = t0; r < K && r < a.o.cap_rows; r += step) {
    const int e = vx_search(a.d.table_offsets, a.d.n, r);
    const int64_t first = a.vnum[2 * vx_clamp(a.d.table_offsets[e], K)];
    const int64_t v0 = vx_vertex(a, 2 * r), v1 = vx_vertex(a, 2 * r + 1);
    a.o.row_vertex[2 * r] = v0 < 0 ? -1 : (int32_t)(v0 - first);
    a.o.row_vertex[2 * r + 1] = v0 < 0 ? -1 : v1 < 0 ? (int32_t)(v0 - first) : (int32_t)(v1 - first);   // a single end point: both
  }
  for (int64_t t = t0; t < a.T; t += step) {
    const vx_u64 key = a.key[t];
    if (key == VX_EMPTY) continue;
    const int64_t v = (int64_t)(key >> 32);
    if (v >= V) continue;
    vx_i64* acc = a.vacc + v * VA;
    const vx_i64 pos = __hip_atomic_fetch_add(acc + A_CURSOR, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const vx_i64 at = a.iscan[v] + pos;
    if (pos < 0 || pos >= acc[A_ROWS] || at < 0 || at >= a.inc_cap) vx_status(a, ST_LOOP);
    else a.seg[at] = (int32_t)t;       // T <= 2^31 slots
  }
}

// ---- launch 10: one thread per incidence: its rank by row inside its segment, then the incidence itself ----------------------------------
__global__ __launch_bounds__(256) void clvtx_rank_kernel(VxArgs a) {
  if (vx_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 256, K = vx_rows(a), V = a.vnum[2 * K];
  int64_t total = a.iscan[V];
  if (total > a.inc_cap) total = a.inc_cap;
  for (int64_t ci = (int64_t)blockIdx.x * 256 + threadIdx.x; ci < total; ci += step) {
    const int64_t t = (int64_t)(uint32_t)a.seg[ci];
    if (t >= a.T) { vx_status(a, ST_LOOP); continue; }
    const vx_u64 key = a.key[t];
    const int64_t v = (int64_t)(key >> 32);
    const uint32_t r = (uint32_t)key;
    if (key == VX_EMPTY || v >= V || r >= K) { vx_status(a, ST_LOOP); continue; }
    const int64_t s0 = a.iscan[v], cnt = a.vacc[v * VA + A_ROWS];
    if (ci < s0 || ci >= s0 + cnt || s0 + cnt > a.inc_cap) { vx_status(a, ST_LOOP); continue; }
    int64_t rank = 0;
    for (int64_t k = 0; k < cnt; ++k) {   // bounded by the vertex's incidences
      const int64_t u = (int64_t)(uint32_t)a.seg[s0 + k];
      if (u < a.T && (uint32_t)a.key[u] < r) ++rank;
    }
    const int64_t at = s0 + rank;
    a.sorted[at] = (int32_t)t;
    if (at < a.o.inc_out_cap) {
      const int e = vx_search(a.d.table_offsets, a.d.n, r);
      const vx_u64 best = a.best[t];
      int64_t* o = a.o.incidence + at * VX_IN;
      o[0] = (int64_t)r - a.d.table_offsets[e], o[1] = a.kind[t], o[2] = a.near[t], o[3] = (int64_t)(best >> 32);
      o[4] = (int64_t)(uint32_t)best;
    }
  }
}

// ---- launch 11: one thread per vertex: its record; the event sums --------------------------------------------------------------------------
__global__ __launch_bounds__(64) void clvtx_vertex_kernel(VxArgs a) {
  __shared__ double u[VX_DIRS * 3][64];   // the end directions of this thread's vertex, in ascending key order
  if (vx_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 64, K = vx_rows(a), V = a.vnum[2 * K];
  const int tx = threadIdx.x;
  for (int64_t v = (int64_t)blockIdx.x * 64 + tx; v < V; v += step) {
    const vx_i64* acc = a.vacc + v * VA;
    const vx_i64 ends = acc[A_ENDS], rows = acc[A_ROWS], bodies = acc[A_BODIES];
    int cnt = 0;
    int64_t hi = a.iscan[v + 1];
    if (hi > a.inc_cap) hi = a.inc_cap;
    for (int64_t i = a.iscan[v]; i < hi && cnt < VX_DIRS; ++i) {   // ascending row = ascending key; bounded by the incidences
      const int64_t t = (int64_t)(uint32_t)a.sorted[i];
      if (t >= a.T) break;
      const int kind = (int)a.kind[t];
      if (!kind) continue;
      const int64_t r = (int64_t)(uint32_t)a.key[t];
      if (r >= K) break;
      const double* ax = a.d.rtab + r * VX_FR + FR_AXIS;
      if (kind & 1) {
        u[cnt * 3][tx] = ax[0], u[cnt * 3 + 1][tx] = ax[1], u[cnt * 3 + 2][tx] = ax[2];
        ++cnt;
      }
      if ((kind & 2) && cnt < VX_DIRS) {
        u[cnt * 3][tx] = -ax[0], u[cnt * 3 + 1][tx] = -ax[1], u[cnt * 3 + 2][tx] = -ax[2];
        ++cnt;
      }
    }
    double lo = 0.0, hi_cos = 0.0;
    bool have = false;
    for (int i = 0; i < cnt; ++i) {        // cnt <= 16: at most 120 pairs
      const double i0 = u[i * 3][tx], i1 = u[i * 3 + 1][tx], i2 = u[i * 3 + 2][tx];
      for (int k = i + 1; k < cnt; ++k) {
        const double c = (i0 * u[k * 3][tx] + i1 * u[k * 3 + 1][tx]) + i2 * u[k * 3 + 2][tx];
        if (!have) lo = hi_cos = c, have = true;
        if (c < lo) lo = c;
        if (c > hi_cos) hi_cos = c;
      }
    }
    const int e = vx_search(a.o.vertex_offsets, a.d.n, v);
    if (v < a.o.cap_vertices) {
      int64_t* t = a.o.vtx_itab + v * VX_VI;
      double* f = a.o.vtx_rtab + v * VX_VR;
      const int s = a.d.ndim == 2 ? 1 : 0;   // 2-D: the volume is (1, s0, s1) in here and x[2] = 0 outside
      t[0] = ends, t[1] = rows, t[2] = bodies, t[3] = acc[A_NEAR], t[4] = acc[A_N], t[5] = acc[A_CHARGE];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bool real = c + s < 3;
        const vx_i64 sum = real ? acc[A_S + c + s] : 0;
        t[6 + c] = sum, t[9 + c] = real ? acc[A_LO + c + s] : 0, t[12 + c] = real ? acc[A_HI + c + s] : 0;
        f[c] = (double)sum / (double)ends;
      }
      t[15] = a.d.itab[(int64_t)(a.vkey[v] >> 1) * VX_FI + FI_END_LO + (a.vkey[v] & 1)];
      t[16] = acc[A_MASK] | (ends > VX_DIRS ? 1ll << 32 : 0);
      f[3] = lo, f[4] = hi_cos;
    }
    vx_add((vx_i64*)a.o.event + (int64_t)e * VX_EV + (ends >= 2 || bodies >= 1 ? 1 : 2), 1);
    vx_max(a.evmax + e, (rows << 32) | acc[A_N]);
  }
}

// ---- launch 12: one thread per vertex: the lowest vertex that holds its event's maximum is the primary ------------------------------------
__global__ __launch_bounds__(256) void clvtx_primary_kernel(VxArgs a) {
  if (vx_overflowed(a)) return;
  const int64_t step = (int64_t)gridDim.x * 256, K = vx_rows(a), V = a.vnum[2 * K];
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += step) {
    const vx_i64* acc = a.vacc + v * VA;
    const int e = vx_search(a.o.vertex_offsets, a.d.n, v);
    if (((acc[A_ROWS] << 32) | acc[A_N]) == a.evmax[e]) vx_min((vx_i64*)a.o.event + (int64_t)e * VX_EV + 3, v - a.o.vertex_offsets[e]);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int64_t vx_slots(int64_t inc_cap) {
  int64_t t = 2;
  while (t < 2 * inc_cap + 2) t <<= 1;
  return t;
}

static size_t vx_layout(int32_t n, int64_t m_total, int64_t inc_cap, VxArgs* a, char* base) {
  const size_t T = (size_t)vx_slots(inc_cap), M2 = 2 * (size_t)(m_total < 1 ? 1 : m_total), I1 = (size_t)(inc_cap < 1 ? 1 : inc_cap);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 7) & ~(size_t)7; return p; };
  char* nclaim = take(8);
  char* key = take(T * 8);
  char* near = take(T * 8);
  char* kind = take(T * 8);
  char* best = take(T * 8);
  char* vacc = take(M2 * VA * 8);
  char* iscan = take((M2 + 1) * 8);
  char* evmax = take((size_t)n * 8);
  char* parent = take(M2 * 4);
  char* root = take(M2 * 4);
  char* vnum = take((M2 + 1) * 4);
  char* vkey = take(M2 * 4);
  char* seg = take(I1 * 4);
  char* sorted = take(I1 * 4);
  char* rbits = take((M2 / 2) * 4);
  if (a) {
    a->nclaim = (vx_i64*)nclaim, a->key = (vx_u64*)key, a->near = (vx_i64*)near, a->kind = (vx_i64*)kind, a->best = (vx_u64*)best;
    a->vacc = (vx_i64*)vacc, a->iscan = (int64_t*)iscan, a->evmax = (vx_i64*)evmax, a->parent = (int32_t*)parent;
    a->root = (int32_t*)root, a->vnum = (int32_t*)vnum, a->vkey = (int32_t*)vkey, a->seg = (int32_t*)seg, a->sorted = (int32_t*)sorted;
    a->rbits = (int32_t*)rbits;
    a->T = (int64_t)T;
    int lg = 0;
    while (((size_t)1 << lg) < T) ++lg;
    a->shift = 64 - lg;
  }
  return off;
}

extern "C" size_t ursn_cluster_vertices_scratch_bytes(int32_t n, int64_t m_total, int64_t inc_cap) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 30) || inc_cap < 0 || inc_cap >= ((int64_t)1 << 30)) return 0;
  return vx_layout(n, m_total, inc_cap, nullptr, nullptr);
}

static unsigned vx_grid(int64_t items, int per, int64_t cap) {
  const int64_t b = cdiv64(items, per);
  return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int ursn_cluster_vertices(const ursn_cluster_vtx_desc* d, const ursn_cluster_vtx_out* out, void* scratch, size_t scratch_bytes,
                                     void* stream) {
  const char* who = "cluster_vertices";
  URSN_REQUIRE(d && out, "%s: null desc / out", who);
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)d->n);
  URSN_REQUIRE(d->m_total >= 0 && d->m_total < ((int64_t)1 << 30), "%s: m_total = %lld outside [0, 2^30)", who, (long long)d->m_total);
  URSN_REQUIRE(d->ndim == 2 || d->ndim == 3, "%s: ndim = %d, expected 2 or 3", who, (int)d->ndim);
  int64_t vol = 1;
  for (int k = 0; k < d->ndim; ++k) {
    URSN_REQUIRE(d->spatial[k] >= 1 && d->spatial[k] <= 32768, "%s: spatial[%d] = %d outside [1, 32768]", who, k, (int)d->spatial[k]);
    vol *= d->spatial[k];
  }
  URSN_REQUIRE(vol < ((int64_t)1 << 31), "%s: %lld voxels, expected fewer than 2^31", who, (long long)vol);
  URSN_REQUIRE(d->radius >= 1 && d->radius <= 3, "%s: radius = %d outside [1, 3]", who, (int)d->radius);
  URSN_REQUIRE(d->min_size >= 1, "%s: min_size = %d < 1", who, (int)d->min_size);
  URSN_REQUIRE(d->inc_cap >= 0 && d->inc_cap < ((int64_t)1 << 30), "%s: inc_cap = %lld outside [0, 2^30)", who, (long long)d->inc_cap);
  URSN_REQUIRE(d->feat_cap >= 0, "%s: feat_cap = %lld < 0", who, (long long)d->feat_cap);
  URSN_REQUIRE(out->cap_rows >= 0, "%s: cap_rows = %lld < 0", who, (long long)out->cap_rows);
  URSN_REQUIRE(out->cap_vertices >= 0, "%s: cap_vertices = %lld < 0", who, (long long)out->cap_vertices);
  URSN_REQUIRE(out->inc_out_cap >= 0, "%s: inc_out_cap = %lld < 0", who, (long long)out->inc_out_cap);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster), "%s: null index / cluster", who);
  URSN_REQUIRE(d->feat_cap == 0 || (d->itab && d->rtab), "%s: null itab / rtab", who);
  URSN_REQUIRE(d->class_mask == 0 || d->cls, "%s: class_mask = 0x%x needs cls", who, (unsigned)d->class_mask);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->vertex_offsets && out->inc_offsets && out->event, "%s: null out->vertex_offsets / out->inc_offsets / out->event", who);
  URSN_REQUIRE(out->cap_vertices == 0 || (out->vtx_itab && out->vtx_rtab), "%s: null out->vtx_itab / out->vtx_rtab", who);
  URSN_REQUIRE(out->inc_out_cap == 0 || out->incidence, "%s: null out->incidence", who);
  URSN_REQUIRE(out->cap_rows == 0 || out->row_vertex, "%s: null out->row_vertex", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)d->itab | (uintptr_t)d->rtab |
                 (uintptr_t)out->vertex_offsets | (uintptr_t)out->vtx_itab | (uintptr_t)out->vtx_rtab | (uintptr_t)out->inc_offsets |
                 (uintptr_t)out->incidence | (uintptr_t)out->event | (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->cluster | (uintptr_t)out->row_vertex | (uintptr_t)out->status) & 3) == 0,
               "%s: index / cluster / row_vertex / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_vertices_scratch_bytes(d->n, d->m_total, d->inc_cap);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  VxArgs a;
  a.d = *d;
  a.o = *out;
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.D0 = d->ndim == 3 ? d->spatial[0] : 1, a.D1 = d->spatial[d->ndim - 2], a.D2 = d->spatial[d->ndim - 1];
  a.V = vol, a.g = d->radius, a.inc_cap = d->inc_cap;
  a.Kmax = M < d->feat_cap ? M : d->feat_cap;
  vx_layout(d->n, M, d->inc_cap, &a, (char*)scratch);
  a.combine = ursn_env_on("URSN_CLVTX_WAVE") ? 1 : 0;   // read at every call: the two routes are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const int64_t keys = 2 * a.Kmax;
  const unsigned walk = a.combine ? vx_grid(keys, 4, VX_WAVE_GRID_CAP) : vx_grid(keys, 256, VX_WAVE_GRID_CAP);
  const int64_t most = a.T > keys ? a.T : keys;
  ursn_note_kernel("clvtx_init");
  hipLaunchKernelGGL(clvtx_init_kernel, dim3(vx_grid(most > d->n ? most : d->n, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_link");
  if (a.combine) hipLaunchKernelGGL(clvtx_link_kernel<true>, dim3(walk), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(clvtx_link_kernel<false>, dim3(walk), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_flatten");
  hipLaunchKernelGGL(clvtx_flatten_kernel, dim3(vx_grid(keys > M ? keys : M, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_scan");
  hipLaunchKernelGGL(clvtx_scan_kernel, dim3(1), dim3(VX_SCAN_THREADS), 0, s, a, 0);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_ends");
  hipLaunchKernelGGL(clvtx_ends_kernel, dim3(vx_grid(keys > d->n ? keys : d->n + 1, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_incidence");
  if (a.combine) hipLaunchKernelGGL(clvtx_incidence_kernel<true>, dim3(walk), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(clvtx_incidence_kernel<false>, dim3(walk), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_slot");
  hipLaunchKernelGGL(clvtx_slot_kernel, dim3(vx_grid(a.T, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_scan");
  hipLaunchKernelGGL(clvtx_scan_kernel, dim3(1), dim3(VX_SCAN_THREADS), 0, s, a, 1);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_drop");
  hipLaunchKernelGGL(clvtx_drop_kernel, dim3(vx_grid(most > d->n ? most : d->n, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_rank");
  hipLaunchKernelGGL(clvtx_rank_kernel, dim3(vx_grid(d->inc_cap, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_vertex");
  hipLaunchKernelGGL(clvtx_vertex_kernel, dim3(vx_grid(keys, 64, VX_GRID_CAP)), dim3(64), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clvtx_primary");
  hipLaunchKernelGGL(clvtx_primary_kernel, dim3(vx_grid(keys, 256, VX_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
