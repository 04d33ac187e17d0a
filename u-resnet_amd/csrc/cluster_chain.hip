// Cluster chains (gfx950): ursn_cluster_chains joins the clusters that are fragments of one broken track.  End points of different
// object records (ursn_cluster_features) that face each other across a gap of at most `max_gap` voxels per axis, with both axes and
// the gap vector collinear within `min_cos`, are JOINED when each is the other's best choice; rows linked by joins form a CHAIN, and
// the chains come back as a second clustering of the same lists in the format ursn_cluster_voxels writes, with a record per chain,
// per join, per row and per event.  include/uresnet_hip.h names the columns; uresnet_amd/clusters.py (cluster_chains_numpy) states
// every field operation by operation, and this file follows it: the same bits.
//
// Why the bits do not move.  Whether a pair of end points is a candidate is decided on coordinates and classes alone, and its three
// cosines are computed from the pair ordered by key, so both end points see the same numbers whichever of them evaluates it.  An end
// point's best is ONE packed minimum, dist2 << 32 | partner key (dist2 <= 2883, a key below 2^31), reduced inside the wave that owns
// the end point: no atomics in the search.  A join is a mutual best, decided per end point from the finished table.  Chains are the
// components of a union-find over rows whose links only ever point at a lower row, so a root is its chain's lowest row whatever the
// order of the unions, and a chain's number is the count of roots before its own.  Everything accumulated across threads is a 64-bit
// INTEGER (atomic add / min / max / or at agent scope).  Every fp64 value is computed by ONE thread (per chain, per join) in the
// statement's order under contract(off); fp64 divide and sqrt are correctly rounded on this device.  No float atomics.
//
// The search does not walk list rows: the gaps are up to 31 voxels and there are at most 2 K end points.  The list positions that
// are end points of eligible rows are marked, counted per tile of 64 entries (a ballot), the tile counts scanned by one workgroup,
// and the end points compacted in list order: the compact array is sorted by event << 32 | index.  For an end point at (x0, x1, x2)
// the end points of plane x0 + d0 with x1 within max_gap are one contiguous range of that array (a 2-D list runs as the volume
// (s0, s1, 1), so its lanes are its rows): one lower-bound binary search, then consecutive compact entries up to the range's last
// index, filtered on x2, the row and the class.  One wave64 per end point, one lane per plane (2 max_gap + 1 <= 63 lanes), then a
// wave reduction of the packed minimum and the accepted count.  URSN_CLCHAIN_WAVE=0 is the plain form: one thread per end point
// takes the planes one after another; the same bits.
//
// Launches: (1) init: the status word (stored once; nothing in this launch ors into it), per row its eligibility, the bits it has to
// report and its cleared tables, the marks cleared; (2) mark: the two end positions of every eligible row; (3) flag: every entry
// with an id checked (its id inside its event's rows, its index inside the volume), the rows' bits reported, the marks counted per
// tile; (4) one workgroup scans the tile counts; (5) compact; (6) search; (7) mutual: the join of an end point, unions of rows;
// (8) two workgroups scan the root flags of the rows and the join flags of the keys; (9) rows: offsets, event records' start, the
// per-row outputs, each row onto its chain's accumulators; (10) entries: merged, and the chain's first position by an atomic minimum;
// (11) one thread per chain: the walk, its record and table row, the event sums; (12) longest, and one thread per join: its record.
// Every loop is bounded: an event search by 17 halvings, a compact search by 32, a plane's range by the end-point count, a
// union-find walk by the row count, the chain walk by the chain's rows.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define CH_FI URSN_CLFEAT_I
#define CH_FR URSN_CLFEAT_R
#define CH_CI URSN_CLCHAIN_CI
#define CH_CR URSN_CLCHAIN_CR
#define CH_JI URSN_CLCHAIN_JI
#define CH_JR URSN_CLCHAIN_JR
#define CH_EV URSN_CLCHAIN_EV
enum { FI_N = 0, FI_CHARGE = 1, FI_LO = 5, FI_HI = 8, FI_FLAGS = 23, FI_END_LO = 24, FI_END_HI = 25, FR_AXIS = 12, FR_LEN = 15 };
enum { A_ROWS = 0, A_JOINS = 1, A_N = 2, A_CHARGE = 3, A_LO = 4, A_HI = 7, A_START = 10, A_G2SUM = 11, A_G2MAX = 12, A_MASK = 13,
       A_FIRST = 14, CA = 15 };
enum { ST_IDS = 1, ST_EMPTY_ROW = 2, ST_INDEX = 4, ST_LOOP = 8, ST_CLASS = 16, ST_END = 32, ST_TABLE = 64 };
#define CH_GRID_CAP 4096       // workgroup cap of the striding kernels
#define CH_WAVE_GRID_CAP 1024  // workgroup cap of the search kernel: 4 end points per workgroup and sweep in the wave form
#define CH_WALK_GRID_CAP 32    // workgroup cap of the chain kernel: 64 chains per workgroup and sweep
#define CH_SCAN_THREADS 1024
#define CH_TILE 64             // list entries per tile of the end-point count: one wave, one ballot
#define CH_BIG (1 << 20)       // above every coordinate

typedef long long ch_i64;
typedef unsigned long long ch_u64;
#define CH_EMPTY (~0ull)
#define CH_NONE INT64_MAX

struct ChArgs {
  ursn_cluster_chain_desc d;
  ursn_cluster_chain_out o;
  int32_t M;          // == d.m_total
  int32_t D0, D1, D2; // the volume as three extents (2-D: s0, s1, 1)
  int32_t g;          // max_gap
  int64_t V;          // D0 D1 D2
  int64_t Kmax;       // min(m_total, feat_cap): no more rows are considered
  int64_t tiles;      // ceil(m_total / CH_TILE)
  int32_t* mark;      // [M1] by list position: the key of the end point there, -1 for none
  int32_t* tcount;    // [tiles] marks per tile
  int32_t* tbase;     // [tiles + 1] exclusive scan: end points before the tile; [tiles] = the end points
  ch_u64* comp;       // [M1] the end points in list order: event << 32 | index
  int32_t* ckey;      // [M1] their keys
  ch_u64* best;       // [2 M1] by key: dist2 << 32 | partner key of the best accepted candidate, CH_EMPTY for none
  int32_t* ncand;     // [2 M1] accepted candidates
  int32_t* partner;   // [2 M1] the key joined to this one, -1 for none
  int32_t* rparent;   // [M1] union-find over rows
  int32_t* rchain;    // [M1] the global chain of a row
  int32_t* rbits;     // [M1] status bits launch 1 found at a row; launch 3 reports them
  int32_t* cnum;      // [M1 + 1] roots before the row = the global chain of a root
  int32_t* crow;      // [M1] the lowest row of a global chain
  int32_t* jnum;      // [2 M1 + 1] joins before the key (a join counts at its lower key)
  int32_t* jkey;      // [M1] the lower key of a global join
  ch_i64* cacc;       // [M1][CA] by global chain
  ch_i64* evmax;      // [n] rows << 32 | n of the event's longest chain
  int wave;
};

#define CH_LOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ void ch_add(ch_i64* p, ch_i64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ch_min(ch_i64* p, ch_i64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ch_max(ch_i64* p, ch_i64 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ch_or(ch_i64* p, ch_i64 v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ch_status(const ChArgs& a, int bits) {
  __hip_atomic_fetch_or(a.o.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows considered: the device-read count, never more than the list could fill or the object tables hold.
__device__ __forceinline__ int64_t ch_rows(const ChArgs& a) {
  const int64_t k = a.d.table_offsets[a.d.n];
  return k < 0 ? 0 : k > a.Kmax ? a.Kmax : k;
}
__device__ __forceinline__ int64_t ch_clamp(int64_t x, int64_t K) { return x < 0 ? 0 : x > K ? K : x; }

// The largest e in [0, n) with off[e] <= x: n <= 65535, at most 16 halvings.
__device__ __forceinline__ int ch_search(const int64_t* off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  for (int s = 0; s < 17 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first compact position in [0, hi) whose word is >= target (hi if none): at most 32 halvings.
__device__ __forceinline__ int ch_lower(const ch_u64* comp, int hi, ch_u64 target) {
  int lo = 0;
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1);
    if (comp[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- union-find over rows (cluster.hip's walk): parent[x] <= x, links only point lower ------------------------------------------------
__device__ __forceinline__ int ch_find(int32_t* parent, int x, int cap, const ChArgs& a) {
  for (int h = 0;; ++h) {
    const int p = CH_LOAD32(parent + x);
    if (p >= x) return x;   // a root
    x = p;
    if (h > cap) {
      ch_status(a, ST_LOOP);
      return -1;
    }
  }
}

__device__ __forceinline__ void ch_union(int32_t* parent, int x, int y, int cap, const ChArgs& a) {
  for (int trip = 0;; ++trip) {
    if (trip > cap) {
      ch_status(a, ST_LOOP);
      return;
    }
    x = ch_find(parent, x, cap, a);
    y = ch_find(parent, y, cap, a);
    if (x < 0 || y < 0 || x == y) return;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) return;   // hi was a root at that instant and now points at lo
    x = old, y = lo;         // hi had a parent already (old < hi): join that with lo
  }
}

// An end point as the cosines need it: its key, coordinates and direction (+axis at the lo end, -axis at the hi end).
struct ChPt {
  int key, x0, x1, x2;
  double u0, u1, u2;
};
__device__ __forceinline__ void ch_coords(const ChArgs& a, int32_t idx, int& x0, int& x1, int& x2) {
  const int plane = a.D1 * a.D2, rem = idx % plane;
  x0 = idx / plane, x1 = rem / a.D2, x2 = rem % a.D2;
}
__device__ __forceinline__ void ch_point(const ChArgs& a, int key, int32_t idx, ChPt& p) {
  p.key = key;
  ch_coords(a, idx, p.x0, p.x1, p.x2);
  const double* ax = a.d.rtab + (int64_t)(key >> 1) * CH_FR + FR_AXIS;
  const bool hi = key & 1;
  p.u0 = hi ? -ax[0] : ax[0], p.u1 = hi ? -ax[1] : ax[1], p.u2 = hi ? -ax[2] : ax[2];
}
__device__ __forceinline__ double ch_axes(const ChPt& p, const ChPt& q) { return -((p.u0 * q.u0 + p.u1 * q.u1) + p.u2 * q.u2); }
// The candidate (p, q), p the lower key: clusters.chain_cosines, line by line.
__device__ __forceinline__ bool ch_cosines(const ChPt& p, const ChPt& q, double min_cos, int& dist2, double& c_ax, double& c_lo,
                                           double& c_hi) {
  const int d0 = q.x0 - p.x0, d1 = q.x1 - p.x1, d2 = q.x2 - p.x2;
  dist2 = d0 * d0 + d1 * d1 + d2 * d2;
  const double s = sqrt((double)dist2), f0 = (double)d0, f1 = (double)d1, f2 = (double)d2;
  c_ax = ch_axes(p, q);
  c_lo = (-((p.u0 * f0 + p.u1 * f1) + p.u2 * f2)) / s;
  c_hi = ((q.u0 * f0 + q.u1 * f1) + q.u2 * f2) / s;
  return c_ax >= min_cos && c_lo >= min_cos && c_hi >= min_cos;
}
// the same from two keys of eligible rows (their end positions were checked by launch 1)
__device__ __forceinline__ void ch_pair(const ChArgs& a, int ka, int kb, ChPt& p, ChPt& q) {
  const int lo = ka < kb ? ka : kb, hi = ka < kb ? kb : ka;
  ch_point(a, lo, a.d.index[a.d.itab[(int64_t)(lo >> 1) * CH_FI + FI_END_LO + (lo & 1)]], p);
  ch_point(a, hi, a.d.index[a.d.itab[(int64_t)(hi >> 1) * CH_FI + FI_END_LO + (hi & 1)]], q);
}

// ---- launch 1: status, per row its eligibility and cleared tables, the marks cleared ------------------------------------------------
__global__ __launch_bounds__(256) void clchain_init_kernel(ChArgs a) {
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
  const int64_t K = ch_rows(a);
  for (int64_t r = t0; r < K; r += step) {
    const int64_t* it = a.d.itab + r * CH_FI;
    const int64_t cnt = it[FI_N], elo = it[FI_END_LO], ehi = it[FI_END_HI];
    const int e = ch_search(a.d.table_offsets, n, r);
    const int64_t tb = a.d.table_offsets[e];
    int bits = 0;
    bool ok = true;
    if (tb > r || r >= a.d.table_offsets[e + 1]) bits |= ST_IDS, ok = false;   // table offsets that do not increase
    else if (cnt <= 0) bits |= ST_EMPTY_ROW, ok = false;                         // not a row ursn_cluster_features wrote
    if (ok && a.d.cls && a.d.cls[r] >= 32) bits |= ST_CLASS, ok = false;
    if (ok && (cnt < a.d.min_size || elo == ehi || (a.d.class_mask && !((a.d.class_mask >> a.d.cls[r]) & 1u)))) ok = false;
    if (ok) {
      const int64_t lo = ch_clamp(a.d.offsets[e], a.M), hi = ch_clamp(a.d.offsets[e + 1], a.M);
      for (int side = 0; side < 2 && ok; ++side) {
        const int64_t p = side ? ehi : elo;
        if (p < lo || p >= hi || a.d.cluster[p] != r - tb) bits |= ST_END, ok = false;
        else if (a.d.index[p] < 0 || a.d.index[p] >= a.V) bits |= ST_INDEX, ok = false;
      }
    }
    a.rbits[r] = bits | (ok ? 1 << 30 : 0);   // bit 30: eligible.  Reported by launch 3: an or here could land before thread 0's store
    a.rparent[r] = (int32_t)r;
    a.rchain[r] = -1;
    for (int side = 0; side < 2; ++side) a.best[2 * r + side] = CH_EMPTY, a.ncand[2 * r + side] = 0, a.partner[2 * r + side] = -1;
    ch_i64* v = a.cacc + r * CA;
    for (int c = 0; c < CA; ++c) v[c] = 0;
    v[A_LO] = v[A_LO + 1] = v[A_LO + 2] = CH_BIG;
    v[A_HI] = v[A_HI + 1] = v[A_HI + 2] = -1;
    v[A_START] = CH_NONE, v[A_FIRST] = CH_NONE;
  }
}

// ---- launch 2: one thread per row: an eligible row marks its two end positions --------------------------------------------------------
__global__ __launch_bounds__(256) void clchain_mark_kernel(ChArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = ch_rows(a);
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < K; r += step) {
    if (!(a.rbits[r] >> 30 & 1)) continue;
    const int64_t* it = a.d.itab + r * CH_FI;
    a.mark[it[FI_END_LO]] = (int32_t)(2 * r), a.mark[it[FI_END_HI]] = (int32_t)(2 * r + 1);   // two members of this row alone
  }
}

// ---- launch 3: the rows' bits; one thread per entry: is it consistent; the marks of its tile counted ----------------------------------
__global__ __launch_bounds__(256) void clchain_flag_kernel(ChArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = ch_rows(a);
  for (int64_t r = t0; r < K; r += step) {
    const int bits = a.rbits[r] & ~(1 << 30);
    if (bits) ch_status(a, bits);
  }
  const int lane = threadIdx.x & 63;
  for (int64_t base = t0 - lane; base < a.M; base += step) {   // uniform per wave: a wave takes one tile per trip
    const int64_t j = base + lane;
    bool marked = false;
    if (j < a.M) {
      marked = a.mark[j] >= 0;
      const int32_t id = a.d.cluster[j];
      if (id != -1) {   // every entry with an id, as the statement checks it
        const int e = ch_search(a.d.offsets, a.d.n, j);
        int bits = 0;
        if (a.d.offsets[e] > j || j >= a.d.offsets[e + 1] || id < 0 || id >= a.d.table_offsets[e + 1] - a.d.table_offsets[e]) bits |= ST_IDS;
        if (a.d.index[j] < 0 || a.d.index[j] >= a.V) bits |= ST_INDEX;
        if (bits) ch_status(a, bits);
      }
    }
    const ch_u64 m = __ballot(marked);
    if (lane == 0) a.tcount[base / CH_TILE] = __popcll(m);
  }
}

// ---- launches 4 and 8: one workgroup per mode: an exclusive scan, a chunk per thread ----------------------------------------------------
// mode 0: the tile counts -> tbase.  mode 1: the root flags of the rows -> cnum, crow.  mode 2: the join flags of the keys -> jnum, jkey.
__device__ __forceinline__ int ch_flag(const ChArgs& a, int mode, int64_t i) {
  return mode == 0 ? a.tcount[i] : mode == 1 ? (a.rparent[i] == i ? 1 : 0) : (a.partner[i] > i ? 1 : 0);
}
__global__ __launch_bounds__(CH_SCAN_THREADS) void clchain_scan_kernel(ChArgs a, int mode0) {
  __shared__ int part[CH_SCAN_THREADS];
  const int mode = mode0 + (int)blockIdx.x;
  const int64_t K = ch_rows(a);
  const int64_t N = mode == 0 ? a.tiles : mode == 1 ? K : 2 * K;
  int32_t* num = mode == 0 ? a.tbase : mode == 1 ? a.cnum : a.jnum;
  int32_t* who = mode == 1 ? a.crow : a.jkey;
  const int64_t per = (N + CH_SCAN_THREADS - 1) / CH_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per < N ? (int64_t)threadIdx.x * per : N, hi = lo + per < N ? lo + per : N;
  int sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += ch_flag(a, mode, i);
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < CH_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunk sums
    const int o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += o;
    __syncthreads();
  }
  int at = part[threadIdx.x] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    const int f = ch_flag(a, mode, i);
    num[i] = at;
    if (mode != 0 && f) who[at] = (int32_t)i;
    at += f;
  }
  if (threadIdx.x == CH_SCAN_THREADS - 1) num[N] = part[threadIdx.x];
}

// ---- launch 5: the end points in list order: event << 32 | index and the key -------------------------------------------------------------
__global__ __launch_bounds__(256) void clchain_compact_kernel(ChArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int lane = threadIdx.x & 63;
  for (int64_t base = t0 - lane; base < a.M; base += step) {   // uniform per wave
    const int64_t j = base + lane;
    const int32_t key = j < a.M ? a.mark[j] : -1;
    const ch_u64 m = __ballot(key >= 0);
    if (key < 0) continue;
    const int64_t at = (int64_t)a.tbase[base / CH_TILE] + __popcll(m & ((1ull << lane) - 1ull));
    const int e = ch_search(a.d.offsets, a.d.n, j);
    a.comp[at] = ((ch_u64)e << 32) | (ch_u64)(uint32_t)a.d.index[j];
    a.ckey[at] = key;
  }
}

// ---- launch 6: the search: the accepted candidates of every end point, counted, and the best of them -----------------------------------
// One plane x0 + d0 around the end point p (compact position `self`, event e): its range of the compact array, every candidate in it.
__device__ __forceinline__ void ch_plane(const ChArgs& a, const ChPt& p, int e, int d0, int E, int& count, ch_u64& best) {
  const int y0 = p.x0 + d0;
  if (y0 < 0 || y0 >= a.D0) return;
  const int lo1 = p.x1 - a.g < 0 ? 0 : p.x1 - a.g, hi1 = p.x1 + a.g > a.D1 - 1 ? a.D1 - 1 : p.x1 + a.g;
  const ch_u64 ev = (ch_u64)e << 32;
  const ch_u64 first = ev | (ch_u64)(((int64_t)y0 * a.D1 + lo1) * a.D2), last = ev | (ch_u64)(((int64_t)y0 * a.D1 + hi1) * a.D2 + a.D2 - 1);
  const int row = p.key >> 1;
  for (int t = ch_lower(a.comp, E, first); t < E; ++t) {   // bounded by the end points
    const ch_u64 w = a.comp[t];
    if (w > last) break;
    const int kq = a.ckey[t];
    if ((kq >> 1) == row) continue;
    const int32_t idx = (int32_t)(uint32_t)w;
    const int z = idx % a.D2 - p.x2;
    if (z > a.g || z < -a.g) continue;
    if (a.d.same_class && a.d.cls[kq >> 1] != a.d.cls[row]) continue;
    ChPt q;
    ch_point(a, kq, idx, q);
    int dist2;
    double c_ax, c_lo, c_hi;
    const bool ok = p.key < kq ? ch_cosines(p, q, a.d.min_cos, dist2, c_ax, c_lo, c_hi) : ch_cosines(q, p, a.d.min_cos, dist2, c_ax, c_lo, c_hi);
    if (!ok) continue;
    ++count;
    const ch_u64 word = ((ch_u64)dist2 << 32) | (ch_u64)(uint32_t)kq;
    if (word < best) best = word;
  }
}

template <bool WAVE>
__global__ __launch_bounds__(256) void clchain_search_kernel(ChArgs a) {
  const int E = a.tbase[a.tiles];
  const int lane = threadIdx.x & 63, w = 2 * a.g + 1;
  const int64_t first = WAVE ? (int64_t)blockIdx.x * 4 : (int64_t)blockIdx.x * 256, sweep = (int64_t)gridDim.x * (WAVE ? 4 : 256);
  for (int64_t base = first; base < E; base += sweep) {   // uniform per workgroup
    const int64_t i = base + (WAVE ? threadIdx.x >> 6 : threadIdx.x);
    if (i >= E) continue;                                  // uniform per wave in the wave form
    const ch_u64 word = a.comp[i];
    const int e = (int)(word >> 32);
    ChPt p;
    ch_point(a, a.ckey[i], (int32_t)(uint32_t)word, p);
    int count = 0;
    ch_u64 best = CH_EMPTY;
    if (WAVE) {
      if (lane < w) ch_plane(a, p, e, lane - a.g, E, count, best);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        count += __shfl_xor(count, d, 64);
        const ch_u64 o = __shfl_xor(best, d, 64);
        if (o < best) best = o;
      }
      if (lane != 0) continue;
    } else {
      for (int d0 = -a.g; d0 <= a.g; ++d0) ch_plane(a, p, e, d0, E, count, best);
    }
    a.best[p.key] = best, a.ncand[p.key] = count;
  }
}

// ---- launch 7: one thread per key: its join, if its best's best is itself; the lower key of a join unites the two rows -----------------
__global__ __launch_bounds__(256) void clchain_mutual_kernel(ChArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = ch_rows(a), keys = 2 * K;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < keys; k += step) {
    const ch_u64 b = a.best[k];
    if (b == CH_EMPTY) continue;
    const int64_t j = (int64_t)(uint32_t)b;
    if (j >= keys || (int64_t)(uint32_t)a.best[j] != k || a.best[j] == CH_EMPTY) continue;
    a.partner[k] = (int32_t)j;
    if (k < j) ch_union(a.rparent, (int)(k >> 1), (int)(j >> 1), (int)K, a);
  }
}

// ---- launch 9: offsets and the event records' start; one thread per row: its outputs, and the row onto its chain ------------------------
__global__ __launch_bounds__(256) void clchain_row_kernel(ChArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = ch_rows(a);
  for (int64_t e = t0; e <= a.d.n; e += step) {
    const int64_t rows = ch_clamp(a.d.table_offsets[e], K);
    a.o.chain_offsets[e] = a.cnum[rows], a.o.join_offsets[e] = a.jnum[2 * rows];
    if (e < a.d.n) {
      const int64_t next = ch_clamp(a.d.table_offsets[e + 1], K);
      const int64_t chains = a.cnum[next] - a.cnum[rows];
      int64_t* ev = a.o.event + e * CH_EV;
      ev[0] = chains, ev[1] = a.jnum[2 * next] - a.jnum[2 * rows], ev[2] = 0, ev[3] = chains > 0 ? INT64_MAX : -1;   // launch 12 lowers [3]
    }
  }
  for (int64_t r = t0; r < K; r += step) {
    const int root = ch_find(a.rparent, (int)r, (int)K, a);
    if (root < 0) continue;   // a walk that ran out: reported
    const int64_t c = a.cnum[root];
    a.rchain[r] = (int32_t)c;
    const int e = ch_search(a.d.table_offsets, a.d.n, r);
    const int64_t tb = a.d.table_offsets[e];
    const int32_t p0 = a.partner[2 * r], p1 = a.partner[2 * r + 1];
    if (r < a.o.cap_rows) {
      a.o.row_chain[r] = (int32_t)(c - a.cnum[ch_clamp(tb, K)]);
      a.o.row_join[2 * r] = p0 < 0 ? -1 : (int32_t)(p0 - 2 * tb), a.o.row_join[2 * r + 1] = p1 < 0 ? -1 : (int32_t)(p1 - 2 * tb);
      a.o.row_candidates[2 * r] = a.ncand[2 * r], a.o.row_candidates[2 * r + 1] = a.ncand[2 * r + 1];
    }
    const int64_t* it = a.d.itab + r * CH_FI;
    ch_i64* acc = a.cacc + c * CA;
    ch_add(acc + A_ROWS, 1);
    ch_add(acc + A_N, it[FI_N]);
    if (it[FI_CHARGE]) ch_add(acc + A_CHARGE, it[FI_CHARGE]);
#pragma unroll
    for (int x = 0; x < 3; ++x) ch_min(acc + A_LO + x, it[FI_LO + x]), ch_max(acc + A_HI + x, it[FI_HI + x]);
    ch_i64 mask = it[FI_FLAGS] != 0 ? 2ll << 32 : 0;
    if (a.d.cls && a.d.cls[r] < 32) mask |= 1ll << a.d.cls[r];
    if (mask) ch_or(acc + A_MASK, mask);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int64_t k = 2 * r + side;
      const int32_t pk = side ? p1 : p0;
      if (pk < 0) {
        ch_min(acc + A_START, k);   // a free end
      } else if (k < pk) {         // a join counts at its lower key
        const ch_i64 d2 = (ch_i64)(a.best[k] >> 32);
        ch_add(acc + A_JOINS, 1), ch_add(acc + A_G2SUM, d2), ch_max(acc + A_G2MAX, d2);
      }
    }
  }
}

// ---- launch 10: one thread per entry: its chain, and its position towards the chain's first -----------------------------------------------
__global__ __launch_bounds__(256) void clchain_entry_kernel(ChArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256, K = ch_rows(a);
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < a.M; j += step) {
    const int32_t id = a.d.cluster[j];
    int32_t out = -1;
    if (id >= 0) {
      const int e = ch_search(a.d.offsets, a.d.n, j);
      const int64_t tb = a.d.table_offsets[e], r = tb + id;
      if (a.d.offsets[e] <= j && j < a.d.offsets[e + 1] && id < a.d.table_offsets[e + 1] - tb && tb >= 0 && r < K && a.rchain[r] >= 0) {
        const int64_t c = a.rchain[r];
        out = (int32_t)(c - a.cnum[ch_clamp(tb, K)]);
        ch_i64* first = a.cacc + c * CA + A_FIRST;
        const ch_i64 local = j - a.d.offsets[e];
        if (local < __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ch_min(first, local);   // it only ever falls
      }
    }
    a.o.merged[j] = out;
  }
}

// ---- launch 11: one thread per chain: the walk; its record and table row; the event sums ----------------------------------------------------
__device__ __forceinline__ int64_t ch_end_pos(const ChArgs& a, int64_t key) { return a.d.itab[(key >> 1) * CH_FI + FI_END_LO + (key & 1)]; }
__global__ __launch_bounds__(64) void clchain_chain_kernel(ChArgs a) {
  const int64_t step = (int64_t)gridDim.x * 64, K = ch_rows(a), C = a.cnum[K];
  for (int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x; c < C; c += step) {
    const ch_i64* acc = a.cacc + c * CA;
    const int64_t r0 = a.crow[c], rows = acc[A_ROWS], joins = acc[A_JOINS];
    const bool ring = acc[A_START] == CH_NONE;
    const int64_t start = ring ? 2 * r0 : acc[A_START];
    double path = 0.0, gaps = 0.0, lowest = 0.0;
    int64_t taken = 0, row = start >> 1, side = start & 1, out = start;
    for (int64_t i = 0; i < rows; ++i) {   // bounded by the chain's rows
      path = path + a.d.rtab[row * CH_FR + FR_LEN];
      out = 2 * row + (1 - side);
      const int32_t pk = a.partner[out];
      if (pk < 0 || taken >= joins) continue;
      ChPt p, q;
      ch_pair(a, (int)out, pk, p, q);
      const double gap = sqrt((double)(ch_i64)(a.best[out] >> 32)), c_ax = ch_axes(p, q);
      path = path + gap;
      gaps = gaps + gap;
      if (taken == 0 || c_ax < lowest) lowest = c_ax;
      ++taken;
      row = pk >> 1, side = pk & 1;
    }
    const int e = ch_search(a.d.table_offsets, a.d.n, r0);
    if (c < a.o.cap_chains) {
      const int64_t end_a = ch_end_pos(a, start), end_b = ch_end_pos(a, out);
      int64_t sq = 0;
      if (end_a >= 0 && end_a < a.M && end_b >= 0 && end_b < a.M) {   // an end position no object record holds: reported, span 0
        int xa0, xa1, xa2, xb0, xb1, xb2;
        ch_coords(a, a.d.index[end_a], xa0, xa1, xa2), ch_coords(a, a.d.index[end_b], xb0, xb1, xb2);
        const int64_t d0 = xa0 - xb0, d1 = xa1 - xb1, d2 = xa2 - xb2;
        sq = d0 * d0 + d1 * d1 + d2 * d2;
      }
      const double span = sqrt((double)sq);
      int64_t* t = a.o.chain_itab + c * CH_CI;
      double* f = a.o.chain_rtab + c * CH_CR;
      t[0] = rows, t[1] = joins, t[2] = acc[A_N], t[3] = acc[A_CHARGE];
#pragma unroll
      for (int x = 0; x < 3; ++x) t[4 + x] = acc[A_LO + x], t[7 + x] = acc[A_HI + x];
      t[10] = r0 - a.d.table_offsets[e], t[11] = end_a, t[12] = end_b, t[13] = acc[A_G2SUM], t[14] = acc[A_G2MAX];
      t[15] = acc[A_MASK] | (ring ? 1ll << 32 : 0);
      f[0] = path, f[1] = gaps, f[2] = span, f[3] = path != 0.0 ? span / path : 0.0, f[4] = lowest;
      a.o.first[c] = acc[A_FIRST] == CH_NONE ? 0 : (int32_t)acc[A_FIRST];
      a.o.size[c] = (int32_t)acc[A_N];
      a.o.cls[c] = a.d.cls ? a.d.cls[r0] : (uint8_t)0;
    }
    if (rows >= 2) ch_add((ch_i64*)a.o.event + (int64_t)e * CH_EV + 2, 1);
    ch_max(a.evmax + e, (rows << 32) | acc[A_N]);
  }
}

// ---- launch 12: one thread per chain: the lowest chain that holds its event's maximum is the longest; one per join: its record -------------
__global__ __launch_bounds__(256) void clchain_final_kernel(ChArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int64_t K = ch_rows(a), C = a.cnum[K], J = a.jnum[2 * K];
  for (int64_t c = t0; c < C; c += step) {
    const ch_i64* acc = a.cacc + c * CA;
    const int e = ch_search(a.d.table_offsets, a.d.n, a.crow[c]);
    if (((acc[A_ROWS] << 32) | acc[A_N]) == a.evmax[e]) ch_min((ch_i64*)a.o.event + (int64_t)e * CH_EV + 3, c - a.o.chain_offsets[e]);
  }
  for (int64_t j = t0; j < J && j < a.o.cap_joins; j += step) {
    const int ka = a.jkey[j], kb = a.partner[ka];
    if (kb < 0) { ch_status(a, ST_LOOP); continue; }   // cannot happen: a join flag is a partner above the key
    const int e = ch_search(a.d.table_offsets, a.d.n, ka >> 1);
    const int64_t tb = a.d.table_offsets[e];
    ChPt p, q;
    ch_pair(a, ka, kb, p, q);
    int dist2;
    double c_ax, c_lo, c_hi;
    ch_cosines(p, q, a.d.min_cos, dist2, c_ax, c_lo, c_hi);
    int64_t* t = a.o.join_itab + j * CH_JI;
    double* f = a.o.join_rtab + j * CH_JR;
    t[0] = ka - 2 * tb, t[1] = kb - 2 * tb, t[2] = dist2, t[3] = ch_end_pos(a, ka), t[4] = ch_end_pos(a, kb);
    t[5] = (int64_t)a.rchain[ka >> 1] - a.o.chain_offsets[e];
    f[0] = c_ax, f[1] = c_lo, f[2] = c_hi, f[3] = sqrt((double)dist2);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static size_t ch_layout(int32_t n, int64_t m_total, ChArgs* a, char* base) {
  const size_t M1 = (size_t)(m_total < 1 ? 1 : m_total), T = (M1 + CH_TILE - 1) / CH_TILE;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 7) & ~(size_t)7; return p; };
  char* comp = take(M1 * 8);
  char* best = take(2 * M1 * 8);
  char* cacc = take(M1 * CA * 8);
  char* evmax = take((size_t)n * 8);
  char* mark = take(M1 * 4);
  char* tcount = take(T * 4);
  char* tbase = take((T + 1) * 4);
  char* ckey = take(M1 * 4);
  char* ncand = take(2 * M1 * 4);
  char* partner = take(2 * M1 * 4);
  char* rparent = take(M1 * 4);
  char* rchain = take(M1 * 4);
  char* rbits = take(M1 * 4);
  char* cnum = take((M1 + 1) * 4);
  char* crow = take(M1 * 4);
  char* jnum = take((2 * M1 + 1) * 4);
  char* jkey = take(M1 * 4);
  if (a) {
    a->comp = (ch_u64*)comp, a->best = (ch_u64*)best, a->cacc = (ch_i64*)cacc, a->evmax = (ch_i64*)evmax, a->mark = (int32_t*)mark;
    a->tcount = (int32_t*)tcount, a->tbase = (int32_t*)tbase, a->ckey = (int32_t*)ckey, a->ncand = (int32_t*)ncand;
    a->partner = (int32_t*)partner, a->rparent = (int32_t*)rparent, a->rchain = (int32_t*)rchain, a->rbits = (int32_t*)rbits;
    a->cnum = (int32_t*)cnum, a->crow = (int32_t*)crow, a->jnum = (int32_t*)jnum, a->jkey = (int32_t*)jkey;
  }
  return off;
}

extern "C" size_t ursn_cluster_chains_scratch_bytes(int32_t n, int64_t m_total) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 30)) return 0;
  return ch_layout(n, m_total, nullptr, nullptr);
}

static unsigned ch_grid(int64_t items, int per, int64_t cap) {
  const int64_t b = cdiv64(items, per);
  return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int ursn_cluster_chains(const ursn_cluster_chain_desc* d, const ursn_cluster_chain_out* out, void* scratch, size_t scratch_bytes,
                                   void* stream) {
  const char* who = "cluster_chains";
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
  URSN_REQUIRE(d->max_gap >= 1 && d->max_gap <= 31, "%s: max_gap = %d outside [1, 31]", who, (int)d->max_gap);
  URSN_REQUIRE(d->min_cos >= 0.0 && d->min_cos <= 1.0, "%s: min_cos = %g outside [0, 1]", who, d->min_cos);   // a NaN fails both
  URSN_REQUIRE(d->min_size >= 1, "%s: min_size = %d < 1", who, (int)d->min_size);
  URSN_REQUIRE(d->same_class == 0 || d->same_class == 1, "%s: same_class = %d, expected 0 or 1", who, (int)d->same_class);
  URSN_REQUIRE(d->feat_cap >= 0, "%s: feat_cap = %lld < 0", who, (long long)d->feat_cap);
  URSN_REQUIRE(out->cap_rows >= 0, "%s: cap_rows = %lld < 0", who, (long long)out->cap_rows);
  URSN_REQUIRE(out->cap_chains >= 0, "%s: cap_chains = %lld < 0", who, (long long)out->cap_chains);
  URSN_REQUIRE(out->cap_joins >= 0, "%s: cap_joins = %lld < 0", who, (long long)out->cap_joins);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster), "%s: null index / cluster", who);
  URSN_REQUIRE(d->feat_cap == 0 || (d->itab && d->rtab), "%s: null itab / rtab", who);
  URSN_REQUIRE(d->class_mask == 0 || d->cls, "%s: class_mask = 0x%x needs cls", who, (unsigned)d->class_mask);
  URSN_REQUIRE(d->same_class == 0 || d->cls, "%s: same_class needs cls", who);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->chain_offsets && out->join_offsets && out->event, "%s: null out->chain_offsets / out->join_offsets / out->event", who);
  URSN_REQUIRE(d->m_total == 0 || out->merged, "%s: null out->merged", who);
  URSN_REQUIRE(out->cap_chains == 0 || (out->chain_itab && out->chain_rtab && out->first && out->size && out->cls),
               "%s: null out->chain_itab / out->chain_rtab / out->first / out->size / out->cls", who);
  URSN_REQUIRE(out->cap_joins == 0 || (out->join_itab && out->join_rtab), "%s: null out->join_itab / out->join_rtab", who);
  URSN_REQUIRE(out->cap_rows == 0 || (out->row_chain && out->row_join && out->row_candidates),
               "%s: null out->row_chain / out->row_join / out->row_candidates", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)d->itab | (uintptr_t)d->rtab |
                 (uintptr_t)out->chain_offsets | (uintptr_t)out->chain_itab | (uintptr_t)out->chain_rtab | (uintptr_t)out->join_offsets |
                 (uintptr_t)out->join_itab | (uintptr_t)out->join_rtab | (uintptr_t)out->event | (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / itab / rtab / the out tables / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->cluster | (uintptr_t)out->merged | (uintptr_t)out->first | (uintptr_t)out->size |
                 (uintptr_t)out->row_chain | (uintptr_t)out->row_join | (uintptr_t)out->row_candidates | (uintptr_t)out->status) & 3) == 0,
               "%s: index / cluster / merged / first / size / the row arrays / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_chains_scratch_bytes(d->n, d->m_total);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  ChArgs a;
  a.d = *d;
  a.o = *out;
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.D0 = d->spatial[0], a.D1 = d->spatial[1], a.D2 = d->ndim == 3 ? d->spatial[2] : 1;
  a.V = vol, a.g = d->max_gap;
  a.Kmax = M < d->feat_cap ? M : d->feat_cap;
  a.tiles = cdiv64(M, CH_TILE);
  ch_layout(d->n, M, &a, (char*)scratch);
  a.wave = ursn_env_on("URSN_CLCHAIN_WAVE") ? 1 : 0;   // read at every call: the two forms are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const int64_t K = a.Kmax, keys = 2 * K;
  const unsigned search = a.wave ? ch_grid(keys, 4, CH_WAVE_GRID_CAP) : ch_grid(keys, 256, CH_WAVE_GRID_CAP);
  const int64_t most = M > d->n + 1 ? M : d->n + 1;
  ursn_note_kernel("clchain_init");
  hipLaunchKernelGGL(clchain_init_kernel, dim3(ch_grid(most, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_mark");
  hipLaunchKernelGGL(clchain_mark_kernel, dim3(ch_grid(K, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_flag");
  hipLaunchKernelGGL(clchain_flag_kernel, dim3(ch_grid(M, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_scan");
  hipLaunchKernelGGL(clchain_scan_kernel, dim3(1), dim3(CH_SCAN_THREADS), 0, s, a, 0);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_compact");
  hipLaunchKernelGGL(clchain_compact_kernel, dim3(ch_grid(M, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_search");
  if (a.wave) hipLaunchKernelGGL(clchain_search_kernel<true>, dim3(search), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(clchain_search_kernel<false>, dim3(search), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_mutual");
  hipLaunchKernelGGL(clchain_mutual_kernel, dim3(ch_grid(keys, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_scan");
  hipLaunchKernelGGL(clchain_scan_kernel, dim3(2), dim3(CH_SCAN_THREADS), 0, s, a, 1);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_row");
  hipLaunchKernelGGL(clchain_row_kernel, dim3(ch_grid(K > d->n + 1 ? K : d->n + 1, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_entry");
  hipLaunchKernelGGL(clchain_entry_kernel, dim3(ch_grid(M, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_chain");
  hipLaunchKernelGGL(clchain_chain_kernel, dim3(ch_grid(K, 64, CH_WALK_GRID_CAP)), dim3(64), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clchain_final");
  hipLaunchKernelGGL(clchain_final_kernel, dim3(ch_grid(K, 256, CH_GRID_CAP)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
