// Cluster cones (gfx950): ursn_cluster_cones gathers the clusters that are fragments of one electromagnetic shower.  A fragment (CHILD,
// represented by the anchor of its object record) looks for the end points (APEXES) of larger rows within `reach` voxels inside whose
// cone of half-angle acos(min_cos) it lies, and LINKS to the nearest; a child large enough to have an axis of its own must also be
// aligned with the apex.  The links form a forest, a SHOWER is a tree, and the showers come back as one more clustering of the same
// lists in the format ursn_cluster_voxels writes, with a record per shower, per link, per row and per event.  include/uresnet_hip.h
// names the columns; uresnet_amd/clusters.py (cluster_cones_numpy) states every field operation by operation, and this file follows
// it: the same bits.
//
// Why the bits do not move.  A candidate's numbers depend on (child, apex) alone, not on which thread evaluates it.  A child's parent
// is ONE packed minimum, dist2 << 32 | apex key (dist2 <= 16129, a key below 2^31), reduced inside the wave that owns the child: no
// atomics in the search.  Parents strictly outrank their children, so the links cannot form a cycle and every row's walk to its root
// ends.  A shower's number is the count of lowest rows of trees before its own.  Everything accumulated across threads is an INTEGER
// (atomic add / min / max / or at agent scope); min_cos and t_max are minima and maxima of strictly positive doubles, taken as 64-bit
// integer min / max on their bit patterns, which order as the doubles do.  Every other fp64 value is computed by ONE thread (per
// link, per shower) in the statement's order under contract(off); fp64 divide and sqrt are correctly rounded on this device.  No
// float atomics.
//
// The search is the chains' search generalised.  The list positions that are apexes of parent-eligible rows are marked, counted per
// tile of 64 entries (a ballot), the tile counts scanned by one workgroup, and the apexes compacted in list order: the compact array
// is sorted by event << 32 | index.  For a child with anchor (m0, m1, m2) the apexes of plane m0 + p with x1 within reach are one
// contiguous range of that array (a 2-D list runs as the volume (s0, s1, 1)): one lower-bound binary search, then consecutive
// compact entries up to the range's last index, filtered on x2, the Euclidean bound, the row, the rank and the class.  One wave64 per
// child row, the lanes STRIDING the 2 reach + 1 <= 255 planes (up to four trips), then a butterfly reduction of the packed minimum and
// the accepted count.  URSN_CLCONE_WAVE=0 is the plain form: one thread per child row takes the planes one after another; the same
// bits.
//
// Launches: (1) init: the status word (stored once; nothing in this launch ors into it), per row its two eligibilities, the bits it
// has to report and its cleared tables, the marks cleared; (2) mark: the two end positions of every parent-eligible row; (3) flag:
// every entry with an id checked, the rows' bits reported, the marks counted per tile; (4) one workgroup scans the tile counts;
// (5) compact; (6) search; (7) walk: per row its root and depth, the row number onto the root's lowest-row slot; (8) two workgroups
// scan the lowest-row flags and the link flags of the rows; (9) rows: offsets, event records' start, the per-row outputs, each row
// onto its shower's accumulators and its parent's child counters; (10) entries: merged, and the shower's first position by an atomic
// minimum; (11) one thread per shower: its record and table row, the event sums; (12) largest, one thread per link: its record, one
// per row: its child counts.  Every loop is bounded: an event search by 17 halvings, a compact search by 32, a plane's range by the
// apex count, the planes by four trips, a walk by the row count.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define CN_FI URSN_CLFEAT_I
#define CN_FR URSN_CLFEAT_R
#define CN_SI URSN_CLCONE_SI
#define CN_SR URSN_CLCONE_SR
#define CN_LI URSN_CLCONE_LI
#define CN_LR URSN_CLCONE_LR
#define CN_EV URSN_CLCONE_EV
enum { FI_N = 0, FI_CHARGE = 1, FI_LO = 5, FI_HI = 8, FI_M = 11, FI_FLAGS = 23, FI_END_LO = 24, FI_END_HI = 25, FR_AXIS = 12 };
enum { A_ROWS = 0, A_N = 1, A_CHARGE = 2, A_LO = 3, A_HI = 6, A_DEPTH = 9, A_D2MAX = 10, A_MASK = 11, A_FIRST = 12, A_MINCOS = 13,
       A_TMAX = 14, A_ROOT = 15, CA = 16 };
enum { ST_IDS = 1, ST_EMPTY_ROW = 2, ST_INDEX = 4, ST_LOOP = 8, ST_CLASS = 16, ST_END = 32, ST_TABLE = 64 };
enum { ROW_CHILD = 1 << 30, ROW_PARENT = 1 << 29 };
#define CN_GRID_CAP 4096       // workgroup cap of the striding kernels
#define CN_WAVE_GRID_CAP 1024  // workgroup cap of the search kernel: 4 child rows per workgroup and sweep in the wave form
#define CN_SCAN_THREADS 1024
#define CN_TILE 64             // list entries per tile of the apex count: one wave, one ballot
#define CN_PLANE_TRIPS 4       // ceil((2 * 127 + 1) / 64): the trips of a wave over a child's planes
#define CN_BIG (1 << 20)       // above every coordinate

typedef long long cn_i64;
typedef unsigned long long cn_u64;
#define CN_EMPTY (~0ull)
#define CN_NONE INT64_MAX

struct CnArgs {
  ursn_cluster_cone_desc d;
  ursn_cluster_cone_out o;
  int32_t M;          // == d.m_total
  int32_t D0, D1, D2; // the volume as three extents (2-D: s0, s1, 1)
  int32_t g;          // reach
  int64_t V;          // D0 D1 D2
  int64_t Kmax;       // min(m_total, feat_cap): no more rows are considered
  int64_t tiles;      // ceil(m_total / CN_TILE)
  int32_t* mark;      // [M1] by list position: the key of the apex there, -1 for none
  int32_t* tcount;    // [tiles] marks per tile
  int32_t* tbase;     // [tiles + 1] exclusive scan: apexes before the tile; [tiles] = the apexes
  cn_u64* comp;       // [M1] the apexes in list order: event << 32 | index
  int32_t* ckey;      // [M1] their keys
  cn_u64* best;       // [M1] by child row: dist2 << 32 | apex key of its link, CN_EMPTY for none
  int32_t* ncand;     // [M1] accepted candidates
  int32_t* rroot;     // [M1] the root of a row's tree, -1 where the walk ran out
  int32_t* rdepth;    // [M1] links to the root
  int32_t* lowrow;    // [M1] by root: the lowest row of its tree
  int32_t* rshower;   // [M1] the global shower of a row
  int32_t* rbits;     // [M1] status bits launch 1 found at a row (launch 3 reports them) | ROW_CHILD | ROW_PARENT
  int32_t* snum;      // [M1 + 1] lowest rows before the row = the global shower of a lowest row
  int32_t* srow;      // [M1] the lowest row of a global shower
  int32_t* lnum;      // [M1 + 1] links before the row
  int32_t* lrow;      // [M1] the child row of a global link
  int32_t* rchild;    // [2 M1] by apex key: direct children
  cn_i64* rchildn;    // [2 M1] by apex key: their summed n
  cn_i64* sacc;       // [M1][CA] by global shower
  cn_i64* evmax;      // [n] rows << 32 | n of the event's largest shower
  int wave;
};

#define CN_LOAD64(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ void cn_add(cn_i64* p, cn_i64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cn_min(cn_i64* p, cn_i64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cn_max(cn_i64* p, cn_i64 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cn_or(cn_i64* p, cn_i64 v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cn_status(const CnArgs& a, int bits) {
  __hip_atomic_fetch_or(a.o.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows considered: the device-read count, never more than the list could fill or the object tables hold.
__device__ __forceinline__ int64_t cn_rows(const CnArgs& a) {
  const int64_t k = a.d.table_offsets[a.d.n];
  return k < 0 ? 0 : k > a.Kmax ? a.Kmax : k;
}
__device__ __forceinline__ int64_t cn_clamp(int64_t x, int64_t K) { return x < 0 ? 0 : x > K ? K : x; }

// The largest e in [0, n) with off[e] <= x: n <= 65535, at most 16 halvings.
__device__ __forceinline__ int cn_search(const int64_t* off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  for (int s = 0; s < 17 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first compact position in [0, hi) whose word is >= target (hi if none): at most 32 halvings.
__device__ __forceinline__ int cn_lower(const cn_u64* comp, int hi, cn_u64 target) {
  int lo = 0;
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1);
    if (comp[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void cn_coords(const CnArgs& a, int32_t idx, int& x0, int& x1, int& x2) {
  const int plane = a.D1 * a.D2, rem = idx % plane;
  x0 = idx / plane, x1 = rem / a.D2, x2 = rem % a.D2;
}

// A child row as the search needs it.
struct CnChild {
  int row, m0, m1, m2;
  int64_t n;
  bool axial;   // itself parent-eligible: its axis is tested too
  double a0, a1, a2;
};
__device__ __forceinline__ void cn_child(const CnArgs& a, int row, CnChild& c) {
  const int64_t* it = a.d.itab + (int64_t)row * CN_FI;
  c.row = row, c.n = it[FI_N];
  c.m0 = (int)it[FI_M], c.m1 = (int)it[FI_M + 1], c.m2 = (int)it[FI_M + 2];   // inside the volume: launch 1 checked it
  c.axial = (a.rbits[row] & ROW_PARENT) != 0;
  const double* ax = a.d.rtab + (int64_t)row * CN_FR + FR_AXIS;
  c.a0 = ax[0], c.a1 = ax[1], c.a2 = ax[2];
}
// The candidate (c, apex key kq at d = m_c - x(apex)): clusters.cone_link, line by line.
__device__ __forceinline__ bool cn_link(const CnArgs& a, const CnChild& c, int kq, int d0, int d1, int d2, int dist2, double& t,
                                        double& c_cone, double& c_ax) {
  const double* ax = a.d.rtab + (int64_t)(kq >> 1) * CN_FR + FR_AXIS;
  const bool hi = kq & 1;
  const double u0 = hi ? -ax[0] : ax[0], u1 = hi ? -ax[1] : ax[1], u2 = hi ? -ax[2] : ax[2];
  const double s = sqrt((double)dist2), f0 = (double)d0, f1 = (double)d1, f2 = (double)d2;
  t = (u0 * f0 + u1 * f1) + u2 * f2;
  c_cone = t / s;
  c_ax = c.axial ? fabs((u0 * c.a0 + u1 * c.a1) + u2 * c.a2) : 0.0;
  return c_cone >= a.d.min_cos && (!c.axial || c_ax >= a.d.min_cos);
}
__device__ __forceinline__ int64_t cn_apex_pos(const CnArgs& a, int64_t key) { return a.d.itab[(key >> 1) * CN_FI + FI_END_LO + (key & 1)]; }
// The link of child row r again, from its packed word (the apex's row is parent-eligible: launch 1 checked its end positions).
__device__ __forceinline__ void cn_relink(const CnArgs& a, int r, cn_u64 word, double& t, double& c_cone, double& c_ax) {
  CnChild c;
  cn_child(a, r, c);
  const int kq = (int)(uint32_t)word;
  int x0, x1, x2;
  cn_coords(a, a.d.index[cn_apex_pos(a, kq)], x0, x1, x2);
  cn_link(a, c, kq, c.m0 - x0, c.m1 - x1, c.m2 - x2, (int)(word >> 32), t, c_cone, c_ax);
}

// ---- launch 1: status, per row its eligibilities and cleared tables, the marks cleared ------------------------------------------------
__global__ __launch_bounds__(256) void clcone_init_kernel(CnArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int n = a.d.n;
  if (t0 == 0) {
    const int64_t k = a.d.table_offsets[n];
    int bits = (k < 0 || k > a.M || a.d.table_offsets[0] != 0 || a.d.offsets[0] != 0 || a.d.offsets[n] != a.M) ? ST_IDS : 0;
    if (k > a.d.feat_cap) bits |= ST_TABLE;
    *a.o.status = bits;
  }
  for (int64_t t = t0; t < a.M; t += step) a.mark[t] = -1;
  for (int64_t t = t0; t < n; t += step) a.evmax[t] = 0;
  const int64_t K = cn_rows(a);
  for (int64_t r = t0; r < K; r += step) {
    const int64_t* it = a.d.itab + r * CN_FI;
    const int64_t cnt = it[FI_N], elo = it[FI_END_LO], ehi = it[FI_END_HI];
    const int e = cn_search(a.d.table_offsets, n, r);
    const int64_t tb = a.d.table_offsets[e];
    int bits = 0;
    bool ok = true;
    if (tb > r || r >= a.d.table_offsets[e + 1]) bits |= ST_IDS, ok = false;   // table offsets that do not increase
    else if (cnt <= 0) bits |= ST_EMPTY_ROW, ok = false;                         // not a row ursn_cluster_features wrote
    if (ok && a.d.cls && a.d.cls[r] >= 32) bits |= ST_CLASS, ok = false;
    if (ok && a.d.class_mask && !((a.d.class_mask >> a.d.cls[r]) & 1u)) ok = false;
    bool child = ok && cnt >= a.d.min_size, parent = ok && cnt >= a.d.seed_size && elo != ehi;
    if (parent) {
      const int64_t lo = cn_clamp(a.d.offsets[e], a.M), hi = cn_clamp(a.d.offsets[e + 1], a.M);
      for (int side = 0; side < 2 && parent; ++side) {
        const int64_t p = side ? ehi : elo;
        if (p < lo || p >= hi || a.d.cluster[p] != r - tb) bits |= ST_END, parent = child = false;
        else if (a.d.index[p] < 0 || a.d.index[p] >= a.V) bits |= ST_INDEX, parent = child = false;
      }
    }
    if (child || parent) {   // the anchor: inside the box of the members, so inside the volume
      const int64_t m0 = it[FI_M], m1 = it[FI_M + 1], m2 = it[FI_M + 2];
      if (m0 < 0 || m0 >= a.D0 || m1 < 0 || m1 >= a.D1 || m2 < 0 || m2 >= a.D2) bits |= ST_END, parent = child = false;
    }
    // Reported by launch 3: an or here could land before thread 0's store
    a.rbits[r] = bits | (child ? ROW_CHILD : 0) | (parent ? ROW_PARENT : 0);
    a.best[r] = CN_EMPTY, a.ncand[r] = 0, a.rroot[r] = -1, a.rdepth[r] = 0, a.lowrow[r] = INT32_MAX, a.rshower[r] = -1;
    for (int side = 0; side < 2; ++side) a.rchild[2 * r + side] = 0, a.rchildn[2 * r + side] = 0;
    cn_i64* v = a.sacc + r * CA;
    for (int c = 0; c < CA; ++c) v[c] = 0;
    v[A_LO] = v[A_LO + 1] = v[A_LO + 2] = CN_BIG;
    v[A_HI] = v[A_HI + 1] = v[A_HI + 2] = -1;
    v[A_FIRST] = CN_NONE, v[A_MINCOS] = CN_NONE;
  }
}

// ---- launch 2: one thread per row: a parent-eligible row marks its two end positions ----------------------------------------------------
__global__ __launch_bounds__(256) void clcone_mark_kernel(CnArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = cn_rows(a);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < K; r += step) {
    if (!(a.rbits[r] & ROW_PARENT)) continue;
    const int64_t* it = a.d.itab + r * CN_FI;
    a.mark[it[FI_END_LO]] = (int32_t)(2 * r), a.mark[it[FI_END_HI]] = (int32_t)(2 * r + 1);   // two members of this row alone
  }
}

// ---- launch 3: the rows' bits; one thread per entry: is it consistent; the marks of its tile counted ----------------------------------
__global__ __launch_bounds__(256) void clcone_flag_kernel(CnArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = cn_rows(a);
  for (int64_t r = t0; r < K; r += step) {
    const int bits = a.rbits[r] & ~(ROW_CHILD | ROW_PARENT);
    if (bits) cn_status(a, bits);
  }
  const int lane = threadIdx.x & 63;
  for (int64_t base = t0 - lane; base < a.M; base += step) {   // uniform per wave: a wave takes one tile per trip
    const int64_t j = base + lane;
    bool marked = false;
    if (j < a.M) {
      marked = a.mark[j] >= 0;
      const int32_t id = a.d.cluster[j];
      if (id != -1) {   // every entry with an id, as the statement checks it
        const int e = cn_search(a.d.offsets, a.d.n, j);
        int bits = 0;
        if (a.d.offsets[e] > j || j >= a.d.offsets[e + 1] || id < 0 || id >= a.d.table_offsets[e + 1] - a.d.table_offsets[e]) bits |= ST_IDS;
        if (a.d.index[j] < 0 || a.d.index[j] >= a.V) bits |= ST_INDEX;
        if (bits) cn_status(a, bits);
      }
    }
    const cn_u64 m = __ballot(marked);
    if (lane == 0) a.tcount[base / CN_TILE] = __popcll(m);
  }
}

// ---- launches 4 and 8: one workgroup per mode: an exclusive scan, a chunk per thread ----------------------------------------------------
// mode 0: the tile counts -> tbase.  mode 1: the lowest-row flags of the rows -> snum, srow.  mode 2: the link flags -> lnum, lrow.
__device__ __forceinline__ int cn_flag(const CnArgs& a, int mode, int64_t i) {
  if (mode == 0) return a.tcount[i];
  if (mode == 2) return a.best[i] != CN_EMPTY ? 1 : 0;
  const int root = a.rroot[i];
  return root >= 0 && a.lowrow[root] == i ? 1 : 0;
}
__global__ __launch_bounds__(CN_SCAN_THREADS) void clcone_scan_kernel(CnArgs a, int mode0) {
  __shared__ int part[CN_SCAN_THREADS];
  const int mode = mode0 + (int)blockIdx.x;
  const int64_t N = mode == 0 ? a.tiles : cn_rows(a);
  int32_t* num = mode == 0 ? a.tbase : mode == 1 ? a.snum : a.lnum;
  int32_t* who = mode == 1 ? a.srow : a.lrow;
  const int64_t per = (N + CN_SCAN_THREADS - 1) / CN_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per < N ? (int64_t)threadIdx.x * per : N, hi = lo + per < N ? lo + per : N;
  int sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += cn_flag(a, mode, i);
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < CN_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunk sums
    const int o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += o;
    __syncthreads();
  }
  int at = part[threadIdx.x] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    const int f = cn_flag(a, mode, i);
    num[i] = at;
    if (mode != 0 && f) who[at] = (int32_t)i;
    at += f;
  }
  if (threadIdx.x == CN_SCAN_THREADS - 1) num[N] = part[threadIdx.x];
}

// ---- launch 5: the apexes in list order: event << 32 | index and the key ------------------------------------------------------------------
__global__ __launch_bounds__(256) void clcone_compact_kernel(CnArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int lane = threadIdx.x & 63;
  for (int64_t base = t0 - lane; base < a.M; base += step) {   // uniform per wave
    const int64_t j = base + lane;
    const int32_t key = j < a.M ? a.mark[j] : -1;
    const cn_u64 m = __ballot(key >= 0);
    if (key < 0) continue;
    const int64_t at = (int64_t)a.tbase[base / CN_TILE] + __popcll(m & ((1ull << lane) - 1ull));
    const int e = cn_search(a.d.offsets, a.d.n, j);
    a.comp[at] = ((cn_u64)e << 32) | (cn_u64)(uint32_t)a.d.index[j];
    a.ckey[at] = key;
  }
}

// ---- launch 6: the search: the accepted candidates of every child row, counted, and the best of them ------------------------------------
// One plane m0 + p around the child c (event e): its range of the compact array, every candidate in it.
__device__ __forceinline__ void cn_plane(const CnArgs& a, const CnChild& c, int e, int p, int E, int& count, cn_u64& best) {
  const int y0 = c.m0 + p;
  if (y0 < 0 || y0 >= a.D0) return;
  const int lo1 = c.m1 - a.g < 0 ? 0 : c.m1 - a.g, hi1 = c.m1 + a.g > a.D1 - 1 ? a.D1 - 1 : c.m1 + a.g;
  const cn_u64 ev = (cn_u64)e << 32;
  const cn_u64 first = ev | (cn_u64)(((int64_t)y0 * a.D1 + lo1) * a.D2), last = ev | (cn_u64)(((int64_t)y0 * a.D1 + hi1) * a.D2 + a.D2 - 1);
  const int g2 = a.g * a.g;
  for (int t = cn_lower(a.comp, E, first); t < E; ++t) {   // bounded by the apexes
    const cn_u64 w = a.comp[t];
    if (w > last) break;
    const int32_t idx = (int32_t)(uint32_t)w;
    const int d2 = c.m2 - idx % a.D2;
    if (d2 > a.g || d2 < -a.g) continue;
    const int d1 = c.m1 - (idx / a.D2) % a.D1, d0 = -p;
    const int dist2 = d0 * d0 + d1 * d1 + d2 * d2;
    if (dist2 < 1 || dist2 > g2) continue;
    const int kq = a.ckey[t], P = kq >> 1;
    if (P == c.row) continue;
    const int64_t nP = a.d.itab[(int64_t)P * CN_FI + FI_N];
    if (!(nP > c.n || (nP == c.n && P < c.row))) continue;   // the parent outranks its child
    if (a.d.same_class && a.d.cls[P] != a.d.cls[c.row]) continue;
    double tt, c_cone, c_ax;
    if (!cn_link(a, c, kq, d0, d1, d2, dist2, tt, c_cone, c_ax)) continue;
    ++count;
    const cn_u64 word = ((cn_u64)dist2 << 32) | (cn_u64)(uint32_t)kq;
    if (word < best) best = word;
  }
}

template <bool WAVE>
__global__ __launch_bounds__(256) void clcone_search_kernel(CnArgs a) {
  const int E = a.tbase[a.tiles];
  const int lane = threadIdx.x & 63, w = 2 * a.g + 1;
  const int64_t K = cn_rows(a);
  const int64_t first = WAVE ? (int64_t)blockIdx.x * 4 : (int64_t)blockIdx.x * 256, sweep = (int64_t)gridDim.x * (WAVE ? 4 : 256);
  for (int64_t base = first; base < K; base += sweep) {   // uniform per workgroup
    const int64_t r = base + (WAVE ? threadIdx.x >> 6 : threadIdx.x);
    if (r >= K || !(a.rbits[r] & ROW_CHILD)) continue;     // uniform per wave in the wave form; launch 1 left no link, no candidate
    const int e = cn_search(a.d.table_offsets, a.d.n, r);
    CnChild c;
    cn_child(a, (int)r, c);
    int count = 0;
    cn_u64 best = CN_EMPTY;
    if (WAVE) {
#pragma unroll 1
      for (int trip = 0; trip < CN_PLANE_TRIPS; ++trip) {   // the lanes stride the planes
        const int p = trip * 64 + lane;
        if (p < w) cn_plane(a, c, e, p - a.g, E, count, best);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        count += __shfl_xor(count, d, 64);
        const cn_u64 o = __shfl_xor(best, d, 64);
        if (o < best) best = o;
      }
      if (lane != 0) continue;
    } else {
      for (int p = -a.g; p <= a.g; ++p) cn_plane(a, c, e, p, E, count, best);
    }
    a.best[r] = best, a.ncand[r] = count;
  }
}

// ---- launch 7: one thread per row: up the parents to the root; the row number onto the root's lowest-row slot --------------------------
__global__ __launch_bounds__(256) void clcone_walk_kernel(CnArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = cn_rows(a);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < K; r += step) {
    int64_t x = r, h = 0;
    for (;; ++h) {   // rank strictly rises: bounded by the rows
      const cn_u64 b = a.best[x];
      if (b == CN_EMPTY) break;
      const int64_t up = (int64_t)((uint32_t)b >> 1);
      if (h >= K || up >= K) {
        cn_status(a, ST_LOOP);
        x = -1;
        break;
      }
      x = up;
    }
    if (x < 0) continue;
    a.rroot[r] = (int32_t)x, a.rdepth[r] = (int32_t)h;
    __hip_atomic_fetch_min(a.lowrow + x, (int32_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- launch 9: offsets and the event records' start; one thread per row: its outputs, the row onto its shower and its parent ------------
__global__ __launch_bounds__(256) void clcone_row_kernel(CnArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = cn_rows(a);
  for (int64_t e = t0; e <= a.d.n; e += step) {
    const int64_t rows = cn_clamp(a.d.table_offsets[e], K);
    a.o.shower_offsets[e] = a.snum[rows], a.o.link_offsets[e] = a.lnum[rows];
    if (e < a.d.n) {
      const int64_t next = cn_clamp(a.d.table_offsets[e + 1], K);
      const int64_t showers = a.snum[next] - a.snum[rows];
      int64_t* ev = a.o.event + e * CN_EV;
      ev[0] = showers, ev[1] = a.lnum[next] - a.lnum[rows], ev[2] = 0, ev[3] = showers > 0 ? INT64_MAX : -1;   // launch 12 lowers [3]
    }
  }
  for (int64_t r = t0; r < K; r += step) {
    const int root = a.rroot[r];
    if (root < 0) continue;   // a walk that ran out: reported
    const int64_t c = a.snum[a.lowrow[root]];
    a.rshower[r] = (int32_t)c;
    const int e = cn_search(a.d.table_offsets, a.d.n, r);
    const int64_t tb = a.d.table_offsets[e];
    const cn_u64 word = a.best[r];
    const bool linked = word != CN_EMPTY;
    const int64_t key = (int64_t)(uint32_t)word;
    if (r < a.o.cap_rows) {
      a.o.row_shower[r] = (int32_t)(c - a.snum[cn_clamp(tb, K)]);
      a.o.row_parent[r] = linked ? (int32_t)(key - 2 * tb) : -1;
      a.o.row_candidates[r] = a.ncand[r];
      a.o.row_depth[r] = a.rdepth[r];
    }
    const int64_t* it = a.d.itab + r * CN_FI;
    cn_i64* acc = a.sacc + c * CA;
    cn_add(acc + A_ROWS, 1);
    cn_add(acc + A_N, it[FI_N]);
    if (it[FI_CHARGE]) cn_add(acc + A_CHARGE, it[FI_CHARGE]);
#pragma unroll
    for (int x = 0; x < 3; ++x) cn_min(acc + A_LO + x, it[FI_LO + x]), cn_max(acc + A_HI + x, it[FI_HI + x]);
    cn_i64 mask = it[FI_FLAGS] != 0 ? 2ll << 32 : 0;
    if (a.d.cls && a.d.cls[r] < 32) mask |= 1ll << a.d.cls[r];
    if (mask) cn_or(acc + A_MASK, mask);
    if (root == r) acc[A_ROOT] = r;   // the one root of this shower
    if (!linked) continue;
    double t, c_cone, c_ax;
    cn_relink(a, (int)r, word, t, c_cone, c_ax);
    cn_max(acc + A_DEPTH, a.rdepth[r]);
    cn_max(acc + A_D2MAX, (cn_i64)(word >> 32));
    cn_min(acc + A_MINCOS, (cn_i64)__double_as_longlong(c_cone));   // strictly positive doubles order as their bit patterns
    cn_max(acc + A_TMAX, (cn_i64)__double_as_longlong(t));
    __hip_atomic_fetch_add(a.rchild + key, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cn_add(a.rchildn + key, it[FI_N]);
  }
}

// ---- launch 10: one thread per entry: its shower, and its position towards the shower's first --------------------------------------------
__global__ __launch_bounds__(256) void clcone_entry_kernel(CnArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = cn_rows(a);
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.M; j += step) {
    const int32_t id = a.d.cluster[j];
    int32_t out = -1;
    if (id >= 0) {
      const int e = cn_search(a.d.offsets, a.d.n, j);
      const int64_t tb = a.d.table_offsets[e], r = tb + id;
      if (a.d.offsets[e] <= j && j < a.d.offsets[e + 1] && id < a.d.table_offsets[e + 1] - tb && tb >= 0 && r < K && a.rshower[r] >= 0) {
        const int64_t c = a.rshower[r];
        out = (int32_t)(c - a.snum[cn_clamp(tb, K)]);
        cn_i64* first = a.sacc + c * CA + A_FIRST;
        const cn_i64 local = j - a.d.offsets[e];
        if (local < CN_LOAD64(first)) cn_min(first, local);   // it only ever falls
      }
    }
    a.o.merged[j] = out;
  }
}

// ---- launch 11: one thread per shower: its record and table row; the event sums ---------------------------------------------------------
__global__ __launch_bounds__(256) void clcone_shower_kernel(CnArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = cn_rows(a), S = a.snum[K];
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < S; c += step) {
    const cn_i64* acc = a.sacc + c * CA;
    const int64_t r0 = a.srow[c], rows = acc[A_ROWS], prim = acc[A_ROOT];
    const int e = cn_search(a.d.table_offsets, a.d.n, r0);
    if (c < a.o.cap_showers) {
      const int64_t tb = a.d.table_offsets[e];
      const int64_t* it = a.d.itab + prim * CN_FI;
      const int64_t k0 = a.rchild[2 * prim], k1 = a.rchild[2 * prim + 1], n0 = a.rchildn[2 * prim], n1 = a.rchildn[2 * prim + 1];
      const bool side = (a.rbits[prim] & ROW_PARENT) && (n1 > n0 || (n1 == n0 && k1 > k0));
      const bool links = rows > 1;
      int64_t* t = a.o.shower_itab + c * CN_SI;
      double* f = a.o.shower_rtab + c * CN_SR;
      t[0] = rows, t[1] = acc[A_N], t[2] = acc[A_CHARGE];
#pragma unroll
      for (int x = 0; x < 3; ++x) t[3 + x] = acc[A_LO + x], t[6 + x] = acc[A_HI + x];
      t[9] = r0 - tb, t[10] = prim - tb, t[11] = it[side ? FI_END_HI : FI_END_LO], t[12] = acc[A_DEPTH], t[13] = acc[A_D2MAX];
      t[14] = it[FI_N], t[15] = acc[A_MASK] | (k0 > 0 && k1 > 0 ? 1ll << 32 : 0);
      f[0] = (double)it[FI_N] / (double)acc[A_N];
      f[1] = links ? __longlong_as_double(acc[A_MINCOS]) : 0.0;
      f[2] = links ? __longlong_as_double(acc[A_TMAX]) : 0.0;
      f[3] = sqrt((double)acc[A_D2MAX]);
      a.o.first[c] = acc[A_FIRST] == CN_NONE ? 0 : (int32_t)acc[A_FIRST];
      a.o.size[c] = (int32_t)acc[A_N];
      a.o.cls[c] = a.d.cls ? a.d.cls[prim] : (uint8_t)0;
    }
    if (rows >= 2) cn_add((cn_i64*)a.o.event + (int64_t)e * CN_EV + 2, 1);
    cn_max(a.evmax + e, (rows << 32) | acc[A_N]);
  }
}

// ---- launch 12: per shower: the lowest that holds its event's maximum is the largest; per link: its record; per row: its children ------
__global__ __launch_bounds__(256) void clcone_final_kernel(CnArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = cn_rows(a), S = a.snum[K], L = a.lnum[K];
  for (int64_t c = t0; c < S; c += step) {
    const cn_i64* acc = a.sacc + c * CA;
    const int e = cn_search(a.d.table_offsets, a.d.n, a.srow[c]);
    if (((acc[A_ROWS] << 32) | acc[A_N]) == a.evmax[e]) cn_min((cn_i64*)a.o.event + (int64_t)e * CN_EV + 3, c - a.o.shower_offsets[e]);
  }
  for (int64_t j = t0; j < L && j < a.o.cap_links; j += step) {
    const int r = a.lrow[j];
    const cn_u64 word = a.best[r];
    if (word == CN_EMPTY) { cn_status(a, ST_LOOP); continue; }   // cannot happen: a link flag is a word
    const int e = cn_search(a.d.table_offsets, a.d.n, r);
    const int64_t tb = a.d.table_offsets[e], key = (int64_t)(uint32_t)word, dist2 = (int64_t)(word >> 32);
    double tt, c_cone, c_ax;
    cn_relink(a, r, word, tt, c_cone, c_ax);
    int64_t* t = a.o.link_itab + j * CN_LI;
    double* f = a.o.link_rtab + j * CN_LR;
    t[0] = r - tb, t[1] = key - 2 * tb, t[2] = dist2, t[3] = cn_apex_pos(a, key);
    t[4] = (int64_t)a.rshower[r] - a.o.shower_offsets[e], t[5] = a.rdepth[r];
    f[0] = c_cone, f[1] = tt, f[2] = sqrt((double)dist2), f[3] = c_ax;
  }
  for (int64_t r = t0; r < K && r < a.o.cap_rows; r += step)
    a.o.row_children[2 * r] = a.rchild[2 * r], a.o.row_children[2 * r + 1] = a.rchild[2 * r + 1];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static size_t cn_layout(int32_t n, int64_t m_total, CnArgs* a, char* base) {
  const size_t M1 = (size_t)(m_total < 1 ? 1 : m_total), T = (M1 + CN_TILE - 1) / CN_TILE;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 7) & ~(size_t)7; return p; };
  char* comp = take(M1 * 8);
  char* best = take(M1 * 8);
  char* sacc = take(M1 * CA * 8);
  char* rchildn = take(2 * M1 * 8);
  char* evmax = take((size_t)n * 8);
  char* mark = take(M1 * 4);
  char* tcount = take(T * 4);
  char* tbase = take((T + 1) * 4);
  char* ckey = take(M1 * 4);
  char* ncand = take(M1 * 4);
  char* rroot = take(M1 * 4);
  char* rdepth = take(M1 * 4);
  char* lowrow = take(M1 * 4);
  char* rshower = take(M1 * 4);
  char* rbits = take(M1 * 4);
  char* snum = take((M1 + 1) * 4);
  char* srow = take(M1 * 4);
  char* lnum = take((M1 + 1) * 4);
  char* lrow = take(M1 * 4);
  char* rchild = take(2 * M1 * 4);
  if (a) {
    a->comp = (cn_u64*)comp, a->best = (cn_u64*)best, a->sacc = (cn_i64*)sacc, a->rchildn = (cn_i64*)rchildn, a->evmax = (cn_i64*)evmax;
    a->mark = (int32_t*)mark, a->tcount = (int32_t*)tcount, a->tbase = (int32_t*)tbase, a->ckey = (int32_t*)ckey;
    a->ncand = (int32_t*)ncand, a->rroot = (int32_t*)rroot, a->rdepth = (int32_t*)rdepth, a->lowrow = (int32_t*)lowrow;
    a->rshower = (int32_t*)rshower, a->rbits = (int32_t*)rbits, a->snum = (int32_t*)snum, a->srow = (int32_t*)srow;
    a->lnum = (int32_t*)lnum, a->lrow = (int32_t*)lrow, a->rchild = (int32_t*)rchild;
  }
  return off;
}

extern "C" size_t ursn_cluster_cones_scratch_bytes(int32_t n, int64_t m_total) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 30)) return 0;
  return cn_layout(n, m_total, nullptr, nullptr);
}

static unsigned cn_grid(int64_t items, int per, int64_t cap) {
  const int64_t b = cdiv64(items, per);
  return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int ursn_cluster_cones(const ursn_cluster_cone_desc* d, const ursn_cluster_cone_out* out, void* scratch, size_t scratch_bytes,
                                  void* stream) {
  const char* who = "cluster_cones";
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
  URSN_REQUIRE(d->reach >= 1 && d->reach <= 127, "%s: reach = %d outside [1, 127]", who, (int)d->reach);
  URSN_REQUIRE(d->min_cos > 0.0 && d->min_cos <= 1.0, "%s: min_cos = %g outside (0, 1]", who, d->min_cos);   // a NaN fails both
  URSN_REQUIRE(d->seed_size >= 2, "%s: seed_size = %d < 2", who, (int)d->seed_size);
  URSN_REQUIRE(d->min_size >= 1, "%s: min_size = %d < 1", who, (int)d->min_size);
  URSN_REQUIRE(d->same_class == 0 || d->same_class == 1, "%s: same_class = %d, expected 0 or 1", who, (int)d->same_class);
  URSN_REQUIRE(d->feat_cap >= 0, "%s: feat_cap = %lld < 0", who, (long long)d->feat_cap);
  URSN_REQUIRE(out->cap_rows >= 0, "%s: cap_rows = %lld < 0", who, (long long)out->cap_rows);
  URSN_REQUIRE(out->cap_showers >= 0, "%s: cap_showers = %lld < 0", who, (long long)out->cap_showers);
  URSN_REQUIRE(out->cap_links >= 0, "%s: cap_links = %lld < 0", who, (long long)out->cap_links);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster), "%s: null index / cluster", who);
  URSN_REQUIRE(d->feat_cap == 0 || (d->itab && d->rtab), "%s: null itab / rtab", who);
  URSN_REQUIRE(d->class_mask == 0 || d->cls, "%s: class_mask = 0x%x needs cls", who, (unsigned)d->class_mask);
  URSN_REQUIRE(d->same_class == 0 || d->cls, "%s: same_class needs cls", who);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->shower_offsets && out->link_offsets && out->event, "%s: null out->shower_offsets / out->link_offsets / out->event", who);
  URSN_REQUIRE(d->m_total == 0 || out->merged, "%s: null out->merged", who);
  URSN_REQUIRE(out->cap_showers == 0 || (out->shower_itab && out->shower_rtab && out->first && out->size && out->cls),
               "%s: null out->shower_itab / out->shower_rtab / out->first / out->size / out->cls", who);
  URSN_REQUIRE(out->cap_links == 0 || (out->link_itab && out->link_rtab), "%s: null out->link_itab / out->link_rtab", who);
  URSN_REQUIRE(out->cap_rows == 0 || (out->row_shower && out->row_parent && out->row_candidates && out->row_children && out->row_depth),
               "%s: null out->row_shower / out->row_parent / out->row_candidates / out->row_children / out->row_depth", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)d->itab | (uintptr_t)d->rtab |
                 (uintptr_t)out->shower_offsets | (uintptr_t)out->shower_itab | (uintptr_t)out->shower_rtab | (uintptr_t)out->link_offsets |
                 (uintptr_t)out->link_itab | (uintptr_t)out->link_rtab | (uintptr_t)out->event | (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->cluster | (uintptr_t)out->merged | (uintptr_t)out->first | (uintptr_t)out->size |
                 (uintptr_t)out->row_shower | (uintptr_t)out->row_parent | (uintptr_t)out->row_candidates | (uintptr_t)out->row_children |
                 (uintptr_t)out->row_depth | (uintptr_t)out->status) & 3) == 0,
               "%s: index / cluster / merged / first / size / the row arrays / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_cones_scratch_bytes(d->n, d->m_total);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  CnArgs a;
  a.d = *d;
  a.o = *out;
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.D0 = d->spatial[0], a.D1 = d->spatial[1], a.D2 = d->ndim == 3 ? d->spatial[2] : 1;
  a.V = vol, a.g = d->reach;
  a.Kmax = M < d->feat_cap ? M : d->feat_cap;
  a.tiles = cdiv64(M, CN_TILE);
  cn_layout(d->n, M, &a, (char*)scratch);
  a.wave = ursn_env_on("URSN_CLCONE_WAVE") ? 1 : 0;   // read at every call: the two forms are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const int64_t K = a.Kmax;
  const unsigned search = a.wave ? cn_grid(K, 4, CN_WAVE_GRID_CAP) : cn_grid(K, 256, CN_WAVE_GRID_CAP);
  const int64_t most = M > d->n + 1 ? M : d->n + 1;
  ursn_note_kernel("clcone_init");
  hipLaunchKernelGGL(clcone_init_kernel, dim3(cn_grid(most, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_mark");
  hipLaunchKernelGGL(clcone_mark_kernel, dim3(cn_grid(K, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_flag");
  hipLaunchKernelGGL(clcone_flag_kernel, dim3(cn_grid(M, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_scan");
  hipLaunchKernelGGL(clcone_scan_kernel, dim3(1), dim3(CN_SCAN_THREADS), 0, s, a, 0);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_compact");
  hipLaunchKernelGGL(clcone_compact_kernel, dim3(cn_grid(M, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_search");
  if (a.wave) hipLaunchKernelGGL(clcone_search_kernel<true>, dim3(search), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(clcone_search_kernel<false>, dim3(search), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_walk");
  hipLaunchKernelGGL(clcone_walk_kernel, dim3(cn_grid(K, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_scan");
  hipLaunchKernelGGL(clcone_scan_kernel, dim3(2), dim3(CN_SCAN_THREADS), 0, s, a, 1);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_row");
  hipLaunchKernelGGL(clcone_row_kernel, dim3(cn_grid(K > d->n + 1 ? K : d->n + 1, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_entry");
  hipLaunchKernelGGL(clcone_entry_kernel, dim3(cn_grid(M, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_shower");
  hipLaunchKernelGGL(clcone_shower_kernel, dim3(cn_grid(K, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clcone_final");
  hipLaunchKernelGGL(clcone_final_kernel, dim3(cn_grid(K, 256, CN_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
