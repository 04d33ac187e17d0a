// Cluster splits (gfx950): ursn_cluster_split cuts a connected component that holds several particles -- the prongs of one vertex,
// two tracks that cross, a track with a hard kink -- at its junctions and kinks, and returns the pieces as one more clustering of the
// same lists in the format ursn_cluster_voxels writes, with a record per piece, per junction, per row and per event.
// include/uresnet_hip.h names the columns; uresnet_amd/clusters.py (cluster_split_numpy) states every field operation by operation,
// and this file follows it: the same bits.
//
// Why the bits do not move.  Whether an entry is cut is a function of the members of its row inside its own ball: integers, and one
// fp64 quotient computed by one thread (the product of the two roots commutes, so the order of the two arms is immaterial).  Pieces
// and junctions are the components of a union-find whose links only ever point at a lower list position, so a root is its
// component's lowest position whatever the order of the unions.  An attachment round reads the stamps of earlier rounds only: a
// stamp is written by its owner alone, and a reader that meets a stamp of the running round treats it like none.  The numberings are
// counts of flags in list order.  Everything accumulated across threads is an INTEGER (32-bit atomic min / add, 64-bit atomic add /
// min / max at agent scope).  A centroid is three divisions by one thread under contract(off).  No float atomics.
//
// The ball as seven words.  The ball of an entry at (x0, x1, x2) with radius r <= 3 is w^3 cells, w = 2 r + 1 <= 7.  Word p holds the
// plane x2 - r + p, bit 8 a + b the cell (x0 - r + a, x1 - r + b): seven rows of seven bits, bit 7 of every byte always clear, so a
// shift by 1 or 8 never carries a cell into a neighbouring row.  (Adjacency is symmetric in the axes, so it does not matter which
// axis the words run along.)  The 3 x 3 x 3 dilation of a set is (h | h << 8 | h >> 8) with h = u | u << 1 | u >> 1 and u the OR of a
// word and its two neighbours; REACH is the centre bit dilated inside the bitmap until nothing changes, the arms are the same flood
// from successive lowest seeds inside REACH & SHELL.  The list row (x0 - r + a, x1 - r + b, x2 - r .. x2 + r) is at most seven
// consecutive entries behind ONE lower-bound binary search; its 7-bit mask of members of the same cluster row is spread over the
// seven words.  Plain form (the default, and URSN_CLSPLIT_WAVE=0): one thread per entry takes the w^2 rows one after another and
// floods its own seven words on the vector unit, 64 entries to an instruction.  Wave form (URSN_CLSPLIT_WAVE=1): one wave64 per
// entry, lane 8 a + b searches its row, and word p is __ballot(bit p of the lane's mask); the searches of a ball then run side by
// side, but the seven words are uniform, so the compiler keeps them in scalar registers and the flood runs on the scalar unit, one
// entry to an instruction.  The whole call measured 1 to 25 % slower that way ("Cluster splits"), so it is not the
// default.  The same words, the same bits.
//
// Launches: (1) init: the status word (stored once; nothing in this launch ors into it), per entry its links and stamps, per row its
// eligibility and cleared counts; (2) flag: every entry checked, its global row, the row's lowest position, eligible entries counted
// per tile of 64 (a ballot); (3) one workgroup scans the tile counts; (4) compact: eligible entries in list order; (5) arms: mark;
// (6) the nine list rows around every entry found and kept, union of adjacent entries of one row with equal cut status; (7) roots;
// (8) `grow` attachment rounds; (9) remainder: junctions that keep entries; (10) piece and junction flags, counted per tile;
// (11) two workgroups scan them; (12) setup: offsets, keys, cleared accumulators; (13) entries: split, and every entry onto its
// piece, junction, row and event; (14) records.  Every loop is bounded: an event search by 17 halvings, a list search by 32, a row
// by 7 (3) entries, a flood by 344 trips, the arms by 15, a union-find walk by the list length.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define SP_PI URSN_CLSPLIT_PI
#define SP_JI URSN_CLSPLIT_JI
#define SP_JR URSN_CLSPLIT_JR
#define SP_ROW URSN_CLSPLIT_ROW
#define SP_EV URSN_CLSPLIT_EV
enum { PA_N = 0, PA_ATT = 1, PA_CONTACTS = 2, PA_JLO = 3, PA_JHI = 4, PA_FIRST = 5, PA = 6 };
enum { JA_ENTRIES = 0, JA_ATT = 1, JA_ARMS = 2, JA_KINKS = 3, JA_S = 4, JA_LO = 7, JA_HI = 10, JA_CONTACTS = 13, JA_PLO = 14, JA_PHI = 15,
       JA = 16 };
enum { ST_IDS = 1, ST_ORDER = 2, ST_INDEX = 4, ST_LOOP = 8, ST_CLASS = 16 };
enum { MK_CUT = 16, MK_KINK = 32, MK_ATT = 64 };
enum { RB_OK = 1 << 29, RB_ELIGIBLE = 1 << 30 };
#define SP_SCAN_THREADS 1024
#define SP_TILE 64              // list entries per tile of a count: one wave, one ballot
#define SP_FLOOD_CAP 344        // a flood adds a cell of at most 343 per trip or ends
#define SP_MAX_ARMS 15
#define SP_BIG (1ll << 40)      // above every coordinate, position and id

typedef long long sp_i64;
typedef unsigned long long sp_u64;

struct SpArgs {
  ursn_cluster_split_desc d;
  ursn_cluster_split_out o;
  int32_t M;            // == d.m_total
  int32_t D0, D1, D2;   // the volume as three extents (2-D: s0, s1, 1)
  int32_t r, w;         // radius, 2 radius + 1
  int64_t V;            // D0 D1 D2
  int64_t tiles;        // ceil(m_total / SP_TILE)
  sp_u64 full, ring;    // the w x w square of a word; its border
  int32_t* vrow;        // [M1] by position: the global row of an entry that takes part, -1 otherwise
  int32_t* rowfirst;    // [M1] by row: its lowest position
  int32_t* rbits;       // [M1] by row: RB_OK | RB_ELIGIBLE | the status bits launch 1 found; launch 2 reports them
  int32_t* rowcnt;      // [M1][3] by row: pieces, junctions, cut entries
  int32_t* tcount;      // [3][tiles] flags per tile: eligible entries, pieces, junctions
  int32_t* tbase;       // [3][tiles + 1] their exclusive scans
  sp_u64* bword;        // [2][tiles] the ballots of the piece and junction flags
  int32_t* comp;        // [M1] the eligible entries in list order
  int32_t* parent;      // [M1] union-find over positions
  int32_t* eroot;       // [M1] the root of an eligible entry, -1 otherwise
  int32_t* stamp;       // [M1] the round that attached a cut entry, 0 for none
  int32_t* apiece;      // [M1] the key of the piece it was attached to
  int32_t* jrem;        // [M1] by position: a junction root that keeps entries after the last round
  int32_t* pkey;        // [M1] by global piece: its key
  int32_t* jkey;        // [M1] by global junction: its lowest position
  int32_t* nbr;         // [M1][9] by position of an eligible entry: where each of the nine list rows around it begins, -1 outside
  sp_i64* pacc;         // [M1][PA]
  sp_i64* jacc;         // [M1][JA]
  sp_i64* evacc;        // [n][2] rows with a junction, cut entries
  int wave;
};

#define SP_LOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define SP_STORE32(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ void sp_add(sp_i64* p, sp_i64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sp_min(sp_i64* p, sp_i64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sp_max(sp_i64* p, sp_i64 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int sp_add32(int32_t* p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sp_status(const SpArgs& a, int bits) {
  __hip_atomic_fetch_or(a.o.status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t sp_clamp(int64_t x, int64_t K) { return x < 0 ? 0 : x > K ? K : x; }
// Rows considered: the device-read count, never more than the list could fill.
__device__ __forceinline__ int64_t sp_rows(const SpArgs& a) { return sp_clamp(a.d.table_offsets[a.d.n], a.M); }

// The largest e in [0, n) with off[e] <= x: n <= 65535, at most 16 halvings.
__device__ __forceinline__ int sp_search(const int64_t* off, int n, int64_t x) {
  int lo = 0, hi = n - 1;
  for (int s = 0; s < 17 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The first position in [lo, hi) whose index is >= target (hi if none): at most 32 halvings.
__device__ __forceinline__ int sp_lower(const int32_t* index, int lo, int hi, int32_t target) {
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1);
    if (index[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- union-find over positions (cluster.hip's walk): parent[x] <= x, links only point lower ---------------------------------------------
__device__ __forceinline__ int sp_find(int32_t* parent, int x, int cap, const SpArgs& a, int* hops) {
  int h = 0;
  for (;;) {
    const int p = SP_LOAD32(parent + x);
    if ((uint32_t)p >= (uint32_t)x) break;   // a root (a word outside [0, x] cannot occur, and the walk stays inside the array if it does)
    x = p;
    if (++h > cap) {
      sp_status(a, ST_LOOP);
      return -1;
    }
  }
  *hops = h;
  return x;
}

__device__ __forceinline__ void sp_union(int32_t* parent, int x, int y, int cap, const SpArgs& a) {
  for (int trip = 0;; ++trip) {
    if (trip > cap) {
      sp_status(a, ST_LOOP);
      return;
    }
    int hx, hy;
    const int x0 = x, y0 = y;
    x = sp_find(parent, x, cap, a, &hx);
    y = sp_find(parent, y, cap, a, &hy);
    if (x < 0 || y < 0) return;
    // shorten the two walked paths: a lower ancestor in place of the parent, by the same monotone atomic as the links
    if (hx > 1) __hip_atomic_fetch_min(parent + x0, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hy > 1) __hip_atomic_fetch_min(parent + y0, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (x == y) return;
    const int hi = x > y ? x : y, lo = x > y ? y : x;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) return;   // hi was a root at that instant and now points at lo
    x = old, y = lo;         // hi had a parent already (old < hi): join that with lo
  }
}

// An entry that takes part: its position, event, the event's range of the list, its global row and coordinates.
struct SpEnt {
  int j, e, lo, hi, row, x0, x1, x2;
};
__device__ __forceinline__ void sp_entry(const SpArgs& a, int j, SpEnt& t) {
  t.j = j;
  t.e = sp_search(a.d.offsets, a.d.n, j);
  t.lo = (int)sp_clamp(a.d.offsets[t.e], a.M), t.hi = (int)sp_clamp(a.d.offsets[t.e + 1], a.M);
  t.row = a.vrow[j];
  const int32_t idx = a.d.index[j];   // inside the volume: launch 2 checked it before it gave the entry a row
  const int plane = a.D1 * a.D2, rem = idx % plane;
  t.x0 = idx / plane, t.x1 = rem / a.D2, t.x2 = rem % a.D2;
}

// The members of t's row among the cells (y0, y1, z0 .. z0 + nz - 1), nz <= 7: bit k = the cell at z0 + k.  Cells outside the volume
// are empty, and the search never leaves the list row (y0, y1): no wrap into another row or plane.
__device__ __forceinline__ uint32_t sp_row_mask(const SpArgs& a, const SpEnt& t, int y0, int y1, int z0, int nz) {
  if (y0 < 0 || y0 >= a.D0 || y1 < 0 || y1 >= a.D1) return 0;
  const int zlo = z0 < 0 ? 0 : z0, zhi = z0 + nz - 1 > a.D2 - 1 ? a.D2 - 1 : z0 + nz - 1;
  if (zlo > zhi) return 0;
  const int32_t base = (int32_t)(((int64_t)y0 * a.D1 + y1) * a.D2);
  const int first = sp_lower(a.d.index, t.lo, t.hi, base + zlo);
  uint32_t m = 0;
  for (int s = 0; s < 7 && first + s < t.hi; ++s) {
    const int32_t idx = a.d.index[first + s];
    if (idx > base + zhi) break;
    if (idx < base + zlo) continue;   // a list that does not increase: reported by launch 2
    if (a.vrow[first + s] == t.row) m |= 1u << (idx - base - z0);
  }
  return m;
}

// The adjacent entries of t's row in ascending position; f(q) returns true to stop.  The nine list rows around an entry are found
// ONCE, by launch 6 (FILL: nine lower-bound searches, their results kept in nbr), and every later walk (the attachment rounds, the
// contacts) starts from the kept positions: nine independent loads in place of nine chains of dependent ones.
template <bool FILL, class F>
__device__ __forceinline__ void sp_neighbours(const SpArgs& a, const SpEnt& t, F f) {
  int32_t* kept = a.nbr + 9 * (int64_t)t.j;
  bool stop = false;
  for (int d0 = -1; d0 <= 1; ++d0)
    for (int d1 = -1; d1 <= 1; ++d1) {
      const int slot = 3 * (d0 + 1) + (d1 + 1);
      const int y0 = t.x0 + d0, y1 = t.x1 + d1;
      const int zlo = t.x2 - 1 < 0 ? 0 : t.x2 - 1, zhi = t.x2 + 1 > a.D2 - 1 ? a.D2 - 1 : t.x2 + 1;
      const bool inside = y0 >= 0 && y0 < a.D0 && y1 >= 0 && y1 < a.D1;   // zlo <= x2 <= zhi always
      const int32_t base = inside ? (int32_t)(((int64_t)y0 * a.D1 + y1) * a.D2) : 0;
      int first;
      if (FILL) {
        first = inside ? sp_lower(a.d.index, t.lo, t.hi, base + zlo) : -1;
        kept[slot] = first;
      } else {
        first = kept[slot];
      }
      if (first < 0 || stop) continue;   // FILL keeps every slot, also after f has asked to stop
      for (int s = 0; s < 3 && first + s < t.hi; ++s) {
        const int q = first + s;
        const int32_t idx = a.d.index[q];
        if (idx > base + zhi) break;
        if (idx < base + zlo || q == t.j || a.vrow[q] != t.row) continue;
        if (f(q)) {
          stop = true;
          break;
        }
      }
    }
}

// ---- the ball as seven words ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ sp_u64 sp_dilate2(sp_u64 u) {
  const sp_u64 h = u | (u << 1) | (u >> 1);
  return h | (h << 8) | (h >> 8);
}
// R grows to everything of `allowed` joined to it by adjacent cells of `allowed` (R is inside `allowed`).  False: the trip cap ran out.
__device__ __forceinline__ bool sp_flood(sp_u64 (&R)[7], const sp_u64 (&allowed)[7]) {
  for (int trip = 0; trip < SP_FLOOD_CAP; ++trip) {
    sp_u64 N[7], changed = 0;
#pragma unroll
    for (int p = 0; p < 7; ++p) {
      const sp_u64 u = R[p] | (p > 0 ? R[p - 1] : 0ull) | (p < 6 ? R[p + 1] : 0ull);
      N[p] = (sp_dilate2(u) & allowed[p]) | R[p];
      changed |= N[p] ^ R[p];
    }
#pragma unroll
    for (int p = 0; p < 7; ++p) R[p] = N[p];
    if (!changed) return true;
  }
  return false;
}
// The sum of x(q) - x(j) over the cells of A: axis 2 runs along the words, axis 0 along the bytes, axis 1 along the bits of a byte.
__device__ __forceinline__ void sp_sums(const sp_u64 (&A)[7], int r, int (&s)[3]) {
  s[0] = s[1] = s[2] = 0;
#pragma unroll
  for (int p = 0; p < 7; ++p) {
    s[2] += __popcll(A[p]) * (p - r);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      s[0] += __popcll(A[p] & (0x7Full << (8 * k))) * (k - r);
      s[1] += __popcll(A[p] & (0x01010101010101ull << k)) * (k - r);
    }
  }
}

// arms | cut << 4 | kink << 5 of the entry whose ball is B.
__device__ __forceinline__ int sp_mark(const SpArgs& a, const sp_u64 (&B)[7]) {
  const int r = a.r, w = a.w;
  sp_u64 R[7], S[7];
#pragma unroll
  for (int p = 0; p < 7; ++p) R[p] = p == r ? 1ull << (9 * r) : 0ull;   // the entry itself: word r, bit 8 r + r
  bool ok = sp_flood(R, B);
#pragma unroll
  for (int p = 0; p < 7; ++p) S[p] = p >= w ? 0ull : R[p] & ((p == 0 || p == w - 1) ? a.full : a.ring);
  int arms = 0, s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  for (int it = 0; it < SP_MAX_ARMS; ++it) {
    int pl = -1;
#pragma unroll
    for (int p = 0; p < 7; ++p)
      if (pl < 0 && S[p]) pl = p;
    if (pl < 0) break;
    sp_u64 A[7];
#pragma unroll
    for (int p = 0; p < 7; ++p) A[p] = p == pl ? S[p] & (~S[p] + 1ull) : 0ull;   // the lowest seed
    ok = sp_flood(A, S) && ok;
#pragma unroll
    for (int p = 0; p < 7; ++p) S[p] &= ~A[p];
    if (arms == 0) sp_sums(A, r, s1);
    else if (arms == 1) sp_sums(A, r, s2);
    ++arms;
  }
  if (!ok) sp_status(a, ST_LOOP);
  bool two = arms == 2;   // exactly two: nothing of the shell is left
#pragma unroll
  for (int p = 0; p < 7; ++p) two = two && S[p] == 0;
  bool kink = false;
  if (two && a.d.kink_cos < 1.0) {
    const int dot = s1[0] * s2[0] + s1[1] * s2[1] + s1[2] * s2[2];
    const int q1 = s1[0] * s1[0] + s1[1] * s1[1] + s1[2] * s1[2], q2 = s2[0] * s2[0] + s2[1] * s2[1] + s2[2] * s2[2];
    if (q1 > 0 && q2 > 0) {
      const double c = (double)dot / (sqrt((double)q1) * sqrt((double)q2));
      kink = c > a.d.kink_cos;
    }
  }
  return arms | ((arms >= 3 || kink) ? MK_CUT : 0) | (kink ? MK_KINK : 0);
}

// ---- launch 1: status, per entry its links and stamps, per row its eligibility and cleared counts ------------------------------------------
__global__ __launch_bounds__(256) void clsplit_init_kernel(SpArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = a.d.n;
  if (t == 0) {
    const int64_t k = a.d.table_offsets[n];
    *a.o.status = (k < 0 || k > a.M || a.d.table_offsets[0] != 0 || a.d.offsets[0] != 0 || a.d.offsets[n] != a.M) ? ST_IDS : 0;
  }
  if (t < a.M) a.parent[t] = (int32_t)t, a.stamp[t] = 0, a.apiece[t] = -1, a.jrem[t] = 0, a.eroot[t] = -1;
  if (t < n) a.evacc[2 * t] = 0, a.evacc[2 * t + 1] = 0;
  if (t < sp_rows(a)) {
    const int e = sp_search(a.d.table_offsets, n, t);
    int bits = 0;
    bool ok = true;
    if (a.d.table_offsets[e] > t || t >= a.d.table_offsets[e + 1]) bits |= ST_IDS, ok = false;   // table offsets that do not increase
    if (ok && a.d.cls && a.d.cls[t] >= 32) bits |= ST_CLASS, ok = false;
    const bool eligible = ok && a.d.size[t] >= a.d.min_size && (!a.d.class_mask || ((a.d.class_mask >> a.d.cls[t]) & 1u));
    a.rbits[t] = bits | (ok ? RB_OK : 0) | (eligible ? RB_ELIGIBLE : 0);   // reported by launch 2: an or here could land before the store
    a.rowfirst[t] = INT32_MAX;
    a.rowcnt[3 * t] = a.rowcnt[3 * t + 1] = a.rowcnt[3 * t + 2] = 0;
  }
}

// ---- launch 2: the rows' bits; one thread per entry: is it consistent, its row, the row's lowest position; eligible entries per tile ------
__global__ __launch_bounds__(256) void clsplit_flag_kernel(SpArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t K = sp_rows(a);
  if (j < K) {
    const int bits = a.rbits[j] & ~(RB_OK | RB_ELIGIBLE);
    if (bits) sp_status(a, bits);
  }
  bool eligible = false;
  if (j < a.M) {
    const int32_t id = a.d.cluster[j], idx = a.d.index[j];
    const int e = sp_search(a.d.offsets, a.d.n, j);
    const bool inside = a.d.offsets[e] <= j && j < a.d.offsets[e + 1];
    int bits = 0, row = -1;
    if (inside && j > a.d.offsets[e] && idx <= a.d.index[j - 1]) bits |= ST_ORDER;
    if (id != -1) {
      const int64_t tb = a.d.table_offsets[e], r = tb + id;
      if (!inside || id < 0 || id >= a.d.table_offsets[e + 1] - tb || tb < 0 || r >= K) bits |= ST_IDS;
      if (idx < 0 || idx >= a.V) bits |= ST_INDEX;
      if (!(bits & (ST_IDS | ST_INDEX)) && (a.rbits[r] & RB_OK)) row = (int)r;
    }
    if (bits) sp_status(a, bits);
    a.vrow[j] = row;
    a.o.mark[j] = 0;
    if (row >= 0) {
      __hip_atomic_fetch_min(a.rowfirst + row, (int32_t)j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      eligible = (a.rbits[row] & RB_ELIGIBLE) != 0;
    }
  }
  const sp_u64 m = __ballot(eligible);
  if ((threadIdx.x & 63) == 0 && j < a.M) a.tcount[j / SP_TILE] = __popcll(m);
}

// ---- launches 3 and 11: one workgroup per mode: an exclusive scan of the tile counts, a chunk per thread ----------------------------------
__global__ __launch_bounds__(SP_SCAN_THREADS) void clsplit_scan_kernel(SpArgs a, int mode0) {
  __shared__ int part[SP_SCAN_THREADS];
  const int mode = mode0 + (int)blockIdx.x;
  const int64_t N = a.tiles;
  const int32_t* cnt = a.tcount + mode * N;
  int32_t* num = a.tbase + mode * (N + 1);
  const int64_t per = (N + SP_SCAN_THREADS - 1) / SP_SCAN_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per < N ? (int64_t)threadIdx.x * per : N, hi = lo + per < N ? lo + per : N;
  int sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += cnt[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < SP_SCAN_THREADS; d <<= 1) {   // inclusive scan of the chunk sums
    const int o = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += o;
    __syncthreads();
  }
  int at = part[threadIdx.x] - sum;
  for (int64_t i = lo; i < hi; ++i) {
    num[i] = at;
    at += cnt[i];
  }
  if (threadIdx.x == SP_SCAN_THREADS - 1) num[N] = part[threadIdx.x];
}

// ---- launch 4: the eligible entries in list order -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clsplit_compact_kernel(SpArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int row = j < a.M ? a.vrow[j] : -1;
  const bool eligible = row >= 0 && (a.rbits[row] & RB_ELIGIBLE);
  const sp_u64 m = __ballot(eligible);
  if (eligible) a.comp[(int64_t)a.tbase[j / SP_TILE] + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)j;
}

// ---- launch 5: the arms of every eligible entry ------------------------------------------------------------------------------------------
template <bool WAVE>
__global__ __launch_bounds__(256) void clsplit_arms_kernel(SpArgs a) {
  const int E = a.tbase[a.tiles];
  const int lane = threadIdx.x & 63;
  const int64_t i = WAVE ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= E) return;   // uniform per wave in the wave form
  SpEnt t;
  sp_entry(a, a.comp[i], t);
  sp_u64 B[7];
  if (WAVE) {
    const int ra = lane >> 3, rb = lane & 7;   // lane 8 a + b owns the list row (x0 - r + a, x1 - r + b)
    const uint32_t m = (ra < a.w && rb < a.w) ? sp_row_mask(a, t, t.x0 - a.r + ra, t.x1 - a.r + rb, t.x2 - a.r, a.w) : 0u;
#pragma unroll
    for (int p = 0; p < 7; ++p) B[p] = __ballot((m >> p) & 1u);
  } else {
#pragma unroll
    for (int p = 0; p < 7; ++p) B[p] = 0;
    for (int ra = 0; ra < a.w; ++ra)
      for (int rb = 0; rb < a.w; ++rb) {
        const uint32_t m = sp_row_mask(a, t, t.x0 - a.r + ra, t.x1 - a.r + rb, t.x2 - a.r, a.w);
#pragma unroll
        for (int p = 0; p < 7; ++p) B[p] |= (sp_u64)((m >> p) & 1u) << (8 * ra + rb);
      }
  }
  const int mark = sp_mark(a, B);
  if (!WAVE || lane == 0) a.o.mark[t.j] = (uint8_t)mark;
}

// ---- launch 6: one thread per eligible entry: its nine list rows found and kept; united with its lower neighbours of equal status ----
__global__ __launch_bounds__(256) void clsplit_union_kernel(SpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.tbase[a.tiles]) return;
  SpEnt t;
  sp_entry(a, a.comp[i], t);
  const int cut = a.o.mark[t.j] & MK_CUT;
  sp_neighbours<true>(a, t, [&](int q) {
    if (q < t.j && (a.o.mark[q] & MK_CUT) == cut) sp_union(a.parent, t.j, q, a.M, a);   // every link from its higher end
    return false;
  });
}

// ---- launch 7: one thread per eligible entry: its root ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clsplit_root_kernel(SpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.tbase[a.tiles]) return;
  const int j = a.comp[i];
  int hops;
  a.eroot[j] = sp_find(a.parent, j, a.M, a, &hops);   // -1: a walk that ran out, reported
}

// ---- launch 8, `grow` times: round t: a cut entry without a piece takes the piece of its lowest neighbour that has one -------------------
__global__ __launch_bounds__(256) void clsplit_attach_kernel(SpArgs a, int round) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.tbase[a.tiles]) return;
  const int j = a.comp[i];
  const int mk = a.o.mark[j];
  if (!(mk & MK_CUT) || a.stamp[j] != 0) return;   // its own stamp: only this thread writes it
  SpEnt t;
  sp_entry(a, j, t);
  int key = -1;
  sp_neighbours<false>(a, t, [&](int q) {
    if (!(a.o.mark[q] & MK_CUT)) {
      key = a.eroot[q];
      return true;
    }
    const int sq = SP_LOAD32(a.stamp + q);   // 0 or this round's: not attached before it
    if (sq >= 1 && sq < round) {
      key = a.apiece[q];                     // written by an earlier launch
      return true;
    }
    return false;
  });
  if (key < 0) return;
  a.apiece[j] = key;
  SP_STORE32(a.stamp + j, round);
  a.o.mark[j] = (uint8_t)(mk | MK_ATT);
}

// ---- launch 9: a junction that keeps an entry after the last round is a piece of kind 2 ----------------------------------------------------
__global__ __launch_bounds__(256) void clsplit_remainder_kernel(SpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.tbase[a.tiles]) return;
  const int j = a.comp[i];
  if ((a.o.mark[j] & MK_CUT) && a.stamp[j] == 0 && a.eroot[j] >= 0) SP_STORE32(a.jrem + a.eroot[j], 1);
}

// ---- launch 10: one thread per entry: is its position the key of a piece, of a junction; both counted per tile ---------------------------
__global__ __launch_bounds__(256) void clsplit_keys_kernel(SpArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool piece = false, junction = false;
  const int row = j < a.M ? a.vrow[j] : -1;
  if (row >= 0) {
    if (!(a.rbits[row] & RB_ELIGIBLE)) piece = a.rowfirst[row] == j;
    else {
      const bool root = a.eroot[j] == j;
      if (a.o.mark[j] & MK_CUT) junction = root, piece = root && a.jrem[j] != 0;
      else piece = root;
    }
  }
  const sp_u64 mp = __ballot(piece), mj = __ballot(junction);
  if ((threadIdx.x & 63) == 0 && j < a.M) {
    const int64_t tile = j / SP_TILE;
    a.bword[tile] = mp, a.bword[a.tiles + tile] = mj;
    a.tcount[a.tiles + tile] = __popcll(mp), a.tcount[2 * a.tiles + tile] = __popcll(mj);
  }
}

// The pieces (which = 0) or junctions (which = 1) whose key is below position p = the global number of the one whose key is p.
__device__ __forceinline__ int64_t sp_number(const SpArgs& a, int which, int64_t p) {
  const int32_t* base = a.tbase + (which + 1) * (a.tiles + 1);
  if (p >= a.M) return base[a.tiles];
  const int64_t tile = p / SP_TILE;
  return (int64_t)base[tile] + __popcll(a.bword[which * a.tiles + tile] & ((1ull << (p & 63)) - 1ull));
}
__device__ __forceinline__ bool sp_is_key(const SpArgs& a, int which, int64_t p) {
  return (a.bword[which * a.tiles + p / SP_TILE] >> (p & 63)) & 1ull;
}

// ---- launch 12: the offsets; one thread per entry: a key names its piece / junction and clears the accumulators ---------------------------
__global__ __launch_bounds__(256) void clsplit_setup_kernel(SpArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j <= a.d.n) {
    const int64_t p = sp_clamp(a.d.offsets[j], a.M);
    a.o.piece_offsets[j] = a.M ? sp_number(a, 0, p) : 0, a.o.junction_offsets[j] = a.M ? sp_number(a, 1, p) : 0;
  }
  if (j >= a.M) return;
  if (sp_is_key(a, 0, j)) {
    const int64_t g = sp_number(a, 0, j);
    a.pkey[g] = (int32_t)j;
    sp_i64* v = a.pacc + g * PA;
    v[PA_N] = v[PA_ATT] = v[PA_CONTACTS] = 0, v[PA_JLO] = SP_BIG, v[PA_JHI] = -1, v[PA_FIRST] = SP_BIG;
  }
  if (sp_is_key(a, 1, j)) {
    const int64_t g = sp_number(a, 1, j);
    a.jkey[g] = (int32_t)j;
    sp_i64* v = a.jacc + g * JA;
    for (int c = 0; c < JA; ++c) v[c] = 0;
    v[JA_LO] = v[JA_LO + 1] = v[JA_LO + 2] = SP_BIG, v[JA_HI] = v[JA_HI + 1] = v[JA_HI + 2] = -1, v[JA_PLO] = SP_BIG, v[JA_PHI] = -1;
  }
}

// ---- launch 13: one thread per entry: its piece, and the entry onto its piece, junction, row and event ------------------------------------
__global__ __launch_bounds__(256) void clsplit_entry_kernel(SpArgs a) {
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j64 >= a.M) return;
  const int j = (int)j64;
  const int row = a.vrow[j];
  if (row < 0) {
    a.o.split[j] = -1;
    return;
  }
  SpEnt t;
  sp_entry(a, j, t);
  const int mk = a.o.mark[j];
  const bool eligible = (a.rbits[row] & RB_ELIGIBLE) != 0, cut = (mk & MK_CUT) != 0, attached = (mk & MK_ATT) != 0;
  const int key = !eligible ? a.rowfirst[row] : attached ? a.apiece[j] : a.eroot[j];
  if (key < 0) {   // a walk that ran out: reported
    a.o.split[j] = -1;
    return;
  }
  const int64_t pbase = sp_number(a, 0, t.lo), jbase = sp_number(a, 1, t.lo);
  const int64_t g = sp_number(a, 0, key);
  a.o.split[j] = (int32_t)(g - pbase);
  sp_i64* pv = a.pacc + g * PA;
  sp_add(pv + PA_N, 1);
  if (attached) sp_add(pv + PA_ATT, 1);
  sp_min(pv + PA_FIRST, j - t.lo);
  if (sp_is_key(a, 0, j)) sp_add32(a.rowcnt + 3 * (int64_t)row, 1);
  if (sp_is_key(a, 1, j) && sp_add32(a.rowcnt + 3 * (int64_t)row + 1, 1) == 0) sp_add(a.evacc + 2 * t.e, 1);
  if (!cut || a.eroot[j] < 0) return;
  const int64_t jg = sp_number(a, 1, a.eroot[j]);
  sp_i64* jv = a.jacc + jg * JA;
  sp_add(jv + JA_ENTRIES, 1);
  if (attached) sp_add(jv + JA_ATT, 1);
  sp_max(jv + JA_ARMS, mk & 15);
  if (mk & MK_KINK) sp_add(jv + JA_KINKS, 1);
  const int x[3] = {t.x0, t.x1, t.x2};
#pragma unroll
  for (int c = 0; c < 3; ++c) sp_add(jv + JA_S + c, x[c]), sp_min(jv + JA_LO + c, x[c]), sp_max(jv + JA_HI + c, x[c]);
  sp_add32(a.rowcnt + 3 * (int64_t)row + 2, 1);
  sp_add(a.evacc + 2 * t.e + 1, 1);
  sp_neighbours<false>(a, t, [&](int q) {   // the contacts of this cut entry
    if ((a.o.mark[q] & MK_CUT) || a.eroot[q] < 0) return false;
    const int64_t pg = sp_number(a, 0, a.eroot[q]);
    sp_add(jv + JA_CONTACTS, 1), sp_min(jv + JA_PLO, pg - pbase), sp_max(jv + JA_PHI, pg - pbase);
    sp_i64* qv = a.pacc + pg * PA;
    sp_add(qv + PA_CONTACTS, 1), sp_min(qv + PA_JLO, jg - jbase), sp_max(qv + PA_JHI, jg - jbase);
    return false;
  });
}

// ---- launch 14: one thread per piece, per junction, per row and per event: the records ---------------------------------------------------
__global__ __launch_bounds__(256) void clsplit_record_kernel(SpArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = a.d.n;
  const int64_t P = a.M ? sp_number(a, 0, a.M) : 0, J = a.M ? sp_number(a, 1, a.M) : 0, K = sp_rows(a);
  if (t < P && t < a.o.cap_pieces) {
    const int key = a.pkey[t], row = a.vrow[key];
    const int e = sp_search(a.d.table_offsets, n, row);
    const sp_i64* v = a.pacc + t * PA;
    const int kind = !(a.rbits[row] & RB_ELIGIBLE) ? 0 : (a.o.mark[key] & MK_CUT) ? 2 : 1;
    int64_t jlo = v[PA_JLO] == SP_BIG ? -1 : v[PA_JLO], jhi = v[PA_JHI];
    if (kind == 2) jlo = jhi = sp_number(a, 1, key) - sp_number(a, 1, sp_clamp(a.d.offsets[e], a.M));
    int64_t* o = a.o.piece_itab + t * SP_PI;
    o[0] = row - a.d.table_offsets[e], o[1] = v[PA_N], o[2] = v[PA_ATT], o[3] = kind, o[4] = key, o[5] = v[PA_CONTACTS], o[6] = jlo, o[7] = jhi;
    a.o.first[t] = v[PA_FIRST] == SP_BIG ? 0 : (int32_t)v[PA_FIRST];
    a.o.size[t] = (int32_t)v[PA_N];
    a.o.cls[t] = a.d.cls ? a.d.cls[row] : (uint8_t)0;
  }
  if (t < J && t < a.o.cap_junctions) {
    const int key = a.jkey[t], row = a.vrow[key];
    const int e = sp_search(a.d.table_offsets, n, row);
    const sp_i64* v = a.jacc + t * JA;
    int64_t* o = a.o.junction_itab + t * SP_JI;
    double* f = a.o.junction_rtab + t * SP_JR;
    o[0] = row - a.d.table_offsets[e], o[1] = v[JA_ENTRIES], o[2] = v[JA_ATT], o[3] = v[JA_ARMS], o[4] = v[JA_KINKS];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[5 + c] = v[JA_S + c], o[8 + c] = v[JA_LO + c], o[11 + c] = v[JA_HI + c];
      f[c] = (double)v[JA_S + c] / (double)v[JA_ENTRIES];
    }
    o[14] = key, o[15] = v[JA_CONTACTS], o[16] = v[JA_PLO] == SP_BIG ? -1 : v[JA_PLO], o[17] = v[JA_PHI];
  }
  if (t < K && t < a.o.cap_rows) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.o.rows[3 * t + c] = a.rowcnt[3 * t + c];
  }
  if (t < n) {
    int64_t* ev = a.o.event + t * SP_EV;
    ev[0] = a.o.piece_offsets[t + 1] - a.o.piece_offsets[t], ev[1] = a.o.junction_offsets[t + 1] - a.o.junction_offsets[t];
    ev[2] = a.evacc[2 * t], ev[3] = a.evacc[2 * t + 1];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static size_t sp_layout(int32_t n, int64_t m_total, SpArgs* a, char* base) {
  const size_t M1 = (size_t)(m_total < 1 ? 1 : m_total), T = (M1 + SP_TILE - 1) / SP_TILE;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 7) & ~(size_t)7; return p; };
  char* pacc = take(M1 * PA * 8);
  char* jacc = take(M1 * JA * 8);
  char* evacc = take((size_t)n * 2 * 8);
  char* bword = take(2 * T * 8);
  char* vrow = take(M1 * 4);
  char* rowfirst = take(M1 * 4);
  char* rbits = take(M1 * 4);
  char* rowcnt = take(M1 * 3 * 4);
  char* tcount = take(3 * T * 4);
  char* tbase = take(3 * (T + 1) * 4);
  char* comp = take(M1 * 4);
  char* parent = take(M1 * 4);
  char* eroot = take(M1 * 4);
  char* stamp = take(M1 * 4);
  char* apiece = take(M1 * 4);
  char* jrem = take(M1 * 4);
  char* pkey = take(M1 * 4);
  char* jkey = take(M1 * 4);
  char* nbr = take(M1 * 9 * 4);
  if (a) {
    a->pacc = (sp_i64*)pacc, a->jacc = (sp_i64*)jacc, a->evacc = (sp_i64*)evacc, a->bword = (sp_u64*)bword, a->vrow = (int32_t*)vrow;
    a->rowfirst = (int32_t*)rowfirst, a->rbits = (int32_t*)rbits, a->rowcnt = (int32_t*)rowcnt, a->tcount = (int32_t*)tcount;
    a->tbase = (int32_t*)tbase, a->comp = (int32_t*)comp, a->parent = (int32_t*)parent, a->eroot = (int32_t*)eroot;
    a->stamp = (int32_t*)stamp, a->apiece = (int32_t*)apiece, a->jrem = (int32_t*)jrem, a->pkey = (int32_t*)pkey, a->jkey = (int32_t*)jkey;
    a->nbr = (int32_t*)nbr;
  }
  return off;
}

extern "C" size_t ursn_cluster_split_scratch_bytes(int32_t n, int64_t m_total) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 30)) return 0;
  return sp_layout(n, m_total, nullptr, nullptr);
}

static unsigned sp_grid(int64_t items, int per) {
  const int64_t b = cdiv64(items, per);
  return (unsigned)(b < 1 ? 1 : b);   // items < 2^30 + 65536: below the grid limit, so no kernel strides
}

extern "C" int ursn_cluster_split(const ursn_cluster_split_desc* d, const ursn_cluster_split_out* out, void* scratch, size_t scratch_bytes,
                                  void* stream) {
  const char* who = "cluster_split";
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
  URSN_REQUIRE(d->kink_cos >= -1.0 && d->kink_cos <= 1.0, "%s: kink_cos = %g outside [-1, 1]", who, d->kink_cos);   // a NaN fails both
  URSN_REQUIRE(d->min_size >= 1, "%s: min_size = %d < 1", who, (int)d->min_size);
  URSN_REQUIRE(d->grow >= 0 && d->grow <= 8, "%s: grow = %d outside [0, 8]", who, (int)d->grow);
  URSN_REQUIRE(d->reserved == 0, "%s: reserved = %d, expected 0", who, (int)d->reserved);
  URSN_REQUIRE(out->cap_pieces >= 0, "%s: cap_pieces = %lld < 0", who, (long long)out->cap_pieces);
  URSN_REQUIRE(out->cap_junctions >= 0, "%s: cap_junctions = %lld < 0", who, (long long)out->cap_junctions);
  URSN_REQUIRE(out->cap_rows >= 0, "%s: cap_rows = %lld < 0", who, (long long)out->cap_rows);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster && d->size), "%s: null index / cluster / size", who);
  URSN_REQUIRE(d->class_mask == 0 || d->cls, "%s: class_mask = 0x%x needs cls", who, (unsigned)d->class_mask);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->piece_offsets && out->junction_offsets && out->event, "%s: null out->piece_offsets / out->junction_offsets / out->event",
               who);
  URSN_REQUIRE(d->m_total == 0 || (out->split && out->mark), "%s: null out->split / out->mark", who);
  URSN_REQUIRE(out->cap_pieces == 0 || (out->piece_itab && out->first && out->size && out->cls),
               "%s: null out->piece_itab / out->first / out->size / out->cls", who);
  URSN_REQUIRE(out->cap_junctions == 0 || (out->junction_itab && out->junction_rtab), "%s: null out->junction_itab / out->junction_rtab", who);
  URSN_REQUIRE(out->cap_rows == 0 || out->rows, "%s: null out->rows", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)out->piece_offsets | (uintptr_t)out->piece_itab |
                 (uintptr_t)out->junction_offsets | (uintptr_t)out->junction_itab | (uintptr_t)out->junction_rtab | (uintptr_t)out->event |
                 (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / the out tables / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->cluster | (uintptr_t)d->size | (uintptr_t)out->split | (uintptr_t)out->first |
                 (uintptr_t)out->size | (uintptr_t)out->rows | (uintptr_t)out->status) & 3) == 0,
               "%s: index / cluster / size / split / first / the row array / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_split_scratch_bytes(d->n, d->m_total);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  SpArgs a;
  a.d = *d;
  a.o = *out;
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.D0 = d->spatial[0], a.D1 = d->spatial[1], a.D2 = d->ndim == 3 ? d->spatial[2] : 1;
  a.V = vol, a.r = d->radius, a.w = 2 * d->radius + 1;
  a.tiles = cdiv64(M, SP_TILE);
  a.full = a.ring = 0;
  for (int ra = 0; ra < a.w; ++ra)
    for (int rb = 0; rb < a.w; ++rb) {
      a.full |= 1ull << (8 * ra + rb);
      if (ra == 0 || rb == 0 || ra == a.w - 1 || rb == a.w - 1) a.ring |= 1ull << (8 * ra + rb);
    }
  sp_layout(d->n, M, &a, (char*)scratch);
  a.wave = ursn_env_set("URSN_CLSPLIT_WAVE") ? 1 : 0;   // opt-in; read at every call: the two forms are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const int64_t most = M > d->n + 1 ? M : d->n + 1;
  const unsigned per_entry = sp_grid(M, 256), all = sp_grid(most, 256);
  ursn_note_kernel("clsplit_init");
  hipLaunchKernelGGL(clsplit_init_kernel, dim3(all), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_flag");
  hipLaunchKernelGGL(clsplit_flag_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_scan");
  hipLaunchKernelGGL(clsplit_scan_kernel, dim3(1), dim3(SP_SCAN_THREADS), 0, s, a, 0);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_compact");
  hipLaunchKernelGGL(clsplit_compact_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_arms");
  if (a.wave) hipLaunchKernelGGL(clsplit_arms_kernel<true>, dim3(sp_grid(M, 4)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(clsplit_arms_kernel<false>, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_union");
  hipLaunchKernelGGL(clsplit_union_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_root");
  hipLaunchKernelGGL(clsplit_root_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  for (int round = 1; round <= d->grow; ++round) {
    ursn_note_kernel("clsplit_attach");
    hipLaunchKernelGGL(clsplit_attach_kernel, dim3(per_entry), dim3(256), 0, s, a, round);
    URSN_HIP(hipGetLastError());
  }
  ursn_note_kernel("clsplit_remainder");
  hipLaunchKernelGGL(clsplit_remainder_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_keys");
  hipLaunchKernelGGL(clsplit_keys_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_scan");
  hipLaunchKernelGGL(clsplit_scan_kernel, dim3(2), dim3(SP_SCAN_THREADS), 0, s, a, 1);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_setup");
  hipLaunchKernelGGL(clsplit_setup_kernel, dim3(all), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_entry");
  hipLaunchKernelGGL(clsplit_entry_kernel, dim3(per_entry), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clsplit_record");
  hipLaunchKernelGGL(clsplit_record_kernel, dim3(all), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
