// Voxel clusters (gfx950): ursn_cluster_voxels labels the connected components of the participating entries of per-event voxel
// lists -- the step every consumer takes after the per-voxel class -- on the sorted lists themselves, so time and scratch scale
// with the list length and never with the volume the indices live in.
//
// Definitions (include/uresnet_hip.h states them in full).  An entry participates when its index lies in [0, prod(spatial)) and its
// class is selected by class_mask.  Two participating entries of ONE event are joined when their coordinates differ by at most 1 on
// every axis and in at most 1 | 2 | 3 axes (3-D connectivity 6 | 18 | 26; 2-D 4 | 8 is 1 | 2 axes), with same_class only when their
// classes are equal.  Adjacency is decided on COORDINATES: indices that differ by 1 across a row end, or by one row across a plane
// end, are not neighbours.  Clusters are the components with at least min_size entries, numbered per event in the order of their
// lowest list position; every other entry gets -1.  first = that lowest position counted from the event's first entry, size = the
// entry count, cls = the class of `first`.
//
// Method.  Union-find over list positions.  The earlier neighbours of an entry lie in the same row (the entry just before it in
// the list) and in up to four earlier rows; a row's candidates are found with one binary search confined to the event's range
// [offsets[e], j) and are then at most three consecutive entries, each compared against the row's own index interval.
//
// THIS FILE USES GLOBAL ATOMICS, unlike its siblings (voxel_io.hip, tiling.hip, symmetry.hip): links are made with 32-bit integer
// atomicMin and sizes are summed with 32-bit integer atomicAdd.  The outputs still do not depend on arrival order: every link goes
// from a higher list position to a lower one, so a component's representative is its LOWEST list position whatever order the merges
// land in; sizes are integer sums; ids come from a scan in list order.  No float atomics.  The same arguments give the same bits.
//
// Visibility across XCDs.  The per-XCD L2s are not coherent, so a load in the merge kernel may see a parent word as it was before
// another XCD's atomic.  The walks read through agent-scope relaxed atomic loads, and the loop tolerates a stale value besides: a
// stale parent is an OLDER link, which still names a true ancestor, so a walk can only end too early, at a node that is no longer a
// root.  The atomicMin's RETURNED value decides: it equals the node only if the node was a root at that instant (the link is made),
// otherwise it names the node's real parent and the loop goes on with that -- a stale read costs a retry, never a wrong link.  All
// words of the merge kernel are written by atomics only.  The flatten, numbering and output passes are later launches.
//
// Every device loop is bounded.  parent[x] <= x always, and pointers only decrease, so a walk from x ends within x steps; in the
// union loop the higher of the two nodes strictly decreases per retry.  Both carry a trip cap of the list length; a thread that
// exceeds it stores a non-zero *status (a vector store) and leaves.  Binary searches run at most 32 halvings.
//
// Launches: init (event of each entry, participation, every x-run folded into its first entry, so a track costs one chain per run
// and not one per voxel), merge, flatten (parent = root, sizes), count / one-workgroup scan / rank (ursn_labels_to_voxels' shape,
// over the "kept representative" flags in list order), output.  The scratch needs no initialisation: every word is written by the
// call before it is read.
#include "ursn_common.h"

#define CL_ITER 8
#define CL_SPAN (256 * CL_ITER)   // list positions per workgroup of the count / rank passes

struct ClArgs {
  ursn_cluster_desc d;
  ursn_cluster_out o;
  int S[3];          // the shape as three axes, last fastest (2-D: a leading axis of extent 1)
  int maxax;         // axes in which two joined entries may differ
  int32_t M;         // == d.m_total
  int64_t B;         // workgroups of the count / rank passes
  int32_t* parent;   // [M] union-find links, parent[x] <= x
  int32_t* sz;       // [M] entries of the component, at its representative
  int32_t* ev;       // [M] event of a participating entry, -1 otherwise
  int32_t* rank;     // [M] kept representatives at earlier positions of the whole list
  int32_t* cnt;      // [B] per-workgroup counts, then exclusive prefixes
  int32_t* total;    // [1] kept representatives of the whole list
};

#define CL_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// The root a walk from x reaches, or -1 (and *status set) when the trip cap ran out.  A word outside [0, x] is treated as a root: it
// cannot occur, and the walk stays inside the array if it does.
__device__ __forceinline__ int cl_find(int32_t* parent, int x, int cap, int32_t* status, int* hops) {
  int h = 0;
  for (;;) {
    const int p = CL_LOAD(parent + x);
    if ((uint32_t)p >= (uint32_t)x) break;
    x = p;
    if (++h > cap) {
      *status = 1;
      return -1;
    }
  }
  *hops = h;
  return x;
}

__device__ __forceinline__ void cl_union(int32_t* parent, int a, int b, int cap, int32_t* status) {
  for (int trip = 0;; ++trip) {
    if (trip > cap) {
      *status = 2;
      return;
    }
    int ha, hb;
    const int a0 = a, b0 = b;
    a = cl_find(parent, a, cap, status, &ha);
    b = cl_find(parent, b, cap, status, &hb);
    if (a < 0 || b < 0) return;
    // shorten the two walked paths: a lower ancestor in place of the parent, by the same monotone atomic as the links
    if (ha > 1) __hip_atomic_fetch_min(parent + a0, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hb > 1) __hip_atomic_fetch_min(parent + b0, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) return;   // hi was a root at that instant and now points at lo
    a = old, b = lo;         // hi had a parent already (old < hi): join that with lo
  }
}

__device__ __forceinline__ bool cl_class_on(uint32_t mask, uint8_t c) { return c < 32 && ((mask >> c) & 1u); }

__device__ __forceinline__ int64_t cl_clamp(int64_t v, int64_t M) { return v < 0 ? 0 : v > M ? M : v; }

// One thread per list position: its event (a binary search over the offsets), whether it participates, and the first entry of its
// x-run -- the stretch of consecutive participating entries (of one class with same_class) at consecutive x in one row.
__global__ __launch_bounds__(256) void cluster_init_kernel(ClArgs a) {
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j64 == 0) *a.o.status = 0;
  if (j64 >= a.M) return;
  const int j = (int)j64;
  int lo = 0, hi = a.d.n - 1;
  for (int s = 0; s < 32 && lo < hi; ++s) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.d.offsets[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  const int64_t e0 = a.d.offsets[lo], e1 = a.d.offsets[lo + 1];
  const uint32_t vox = (uint32_t)a.S[0] * (uint32_t)a.S[1] * (uint32_t)a.S[2];
  const int32_t idx = a.d.index[j];
  const uint8_t c = a.d.cls[j];
  const bool part = e0 <= j && j < e1 && (uint32_t)idx < vox && cl_class_on(a.d.class_mask, c);
  int start = j;
  if (part) {
    const int64_t first = e0 > 0 ? e0 : 0;
    const int x2 = (int)((uint32_t)idx % (uint32_t)a.S[2]);
    for (int k = 1; k <= x2 && j - k >= first; ++k) {   // at most x2 < spatial's last extent steps, and never past the event's start
      const int q = j - k;
      if (a.d.index[q] != idx - k) break;
      const uint8_t cq = a.d.cls[q];
      if (!cl_class_on(a.d.class_mask, cq) || (a.d.same_class && cq != c)) break;
      start = q;
    }
  }
  a.parent[j] = start;
  a.sz[j] = 0;
  a.ev[j] = part ? lo : -1;
}

// Four threads per participating entry, one per earlier row that can hold neighbours: (x0 - 1, x1 - 1 | x1 | x1 + 1) and
// (x0, x1 - 1).  A thread joins the entry with its neighbours in that row; the same-row neighbour is the x-run the init pass folded.
// (A thread per row, not per entry: the binary search is a chain of dependent loads, and four chains side by side cost one.)
__global__ __launch_bounds__(256) void cluster_merge_kernel(ClArgs a) {
  const int64_t t64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j64 = t64 >> 2;
  if (j64 >= a.M) return;
  const int j = (int)j64, r = (int)(t64 & 3);
  const int e = a.ev[j];
  if (e < 0) return;
  const int lo = (int)cl_clamp(a.d.offsets[e], a.M);
  const uint32_t idx = (uint32_t)a.d.index[j];
  const uint8_t c = a.d.cls[j];
  const uint32_t S1 = (uint32_t)a.S[1], S2 = (uint32_t)a.S[2], plane = S1 * S2;
  const int x0 = (int)(idx / plane), x1 = (int)((idx - (uint32_t)x0 * plane) / S2), x2 = (int)(idx % S2);
  const int cap = a.M;
  const int d0 = r < 3 ? -1 : 0, d1 = r < 3 ? r - 1 : -1;
  const int nz = (d0 != 0) + (d1 != 0);
  if (nz > a.maxax) return;
  const int y0 = x0 + d0, y1 = x1 + d1;
  if (y0 < 0 || y1 < 0 || y1 >= a.S[1]) return;
  const int w = nz < a.maxax ? 1 : 0;
  const int zlo = x2 - w < 0 ? 0 : x2 - w, zhi = x2 + w > a.S[2] - 1 ? a.S[2] - 1 : x2 + w;
  const int32_t base = (int32_t)(((uint32_t)y0 * S1 + (uint32_t)y1) * S2);
  const int32_t klo = base + zlo, khi = base + zhi;   // the neighbouring row's own interval: no wrap into another row or plane
  int L = lo, H = j;
  for (int s = 0; s < 32 && L < H; ++s) {
    const int mid = L + ((H - L) >> 1);
    if (a.d.index[mid] < klo) L = mid + 1;
    else H = mid;
  }
  int32_t prev = -2;
  for (int t = 0; t < 3; ++t) {
    const int q = L + t;
    if (q >= j) break;
    const int32_t iq = a.d.index[q];
    if (iq < klo || iq > khi) break;
    if (a.ev[q] < 0) continue;
    if (a.d.same_class && a.d.cls[q] != c) continue;
    const bool same_run = prev == iq - 1;   // x-neighbour of the entry just joined: one x-run, already one set
    prev = iq;
    if (!same_run) cl_union(a.parent, j, q, cap, a.o.status);
  }
}

// One thread per participating entry: parent = root (relaxed agent-scope stores, like every access to a parent word while walks run:
// a concurrent walk that reads the old or the new word sees a true ancestor either way), and the component sizes.  Consecutive lanes with one root are counted by ballot, the stretches of a workgroup
// that share a root are added up in a 256-slot LDS table (open addressing, at most 256 stretches: it cannot fill up, and a probe
// walk is capped at 256 slots), and each distinct root of the workgroup costs ONE global integer add: a giant component is a few
// thousand adds to its word, not one per entry.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(ClArgs a) {
  __shared__ int32_t tkey[256], tval[256];
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  tkey[threadIdx.x] = -1;
  tval[threadIdx.x] = 0;
  __syncthreads();
  bool act = j64 < a.M && a.ev[j64 < a.M ? j64 : 0] >= 0;
  int r = -1;
  if (act) {
    int h;
    r = cl_find(a.parent, (int)j64, a.M, a.o.status, &h);
    if (r < 0) act = false;
    else if (h > 1) __hip_atomic_store(a.parent + j64, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int up = __shfl_up(r, 1, 64);
  const bool lead = act && (lane == 0 || up != r);
  const unsigned long long ml = __ballot(lead), ma = __ballot(act);
  if (lead) {
    const unsigned long long above = ~((2ull << lane) - 1ull);   // lanes above this one (lane 63: none)
    const unsigned long long nb = (ml | ~ma) & above;
    const int end = nb ? __ffsll((long long)nb) - 1 : 64;
    uint32_t slot = ((uint32_t)r * 2654435761u) >> 24;
    for (int probe = 0; probe < 256; ++probe, slot = (slot + 1) & 255) {
      const int32_t old = atomicCAS(&tkey[slot], -1, r);
      if (old == -1 || old == r) {
        atomicAdd(&tval[slot], end - lane);
        break;
      }
    }
  }
  __syncthreads();
  const int32_t key = tkey[threadIdx.x];
  if (key >= 0) __hip_atomic_fetch_add(a.sz + key, tval[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool cl_kept_rep(const ClArgs& a, int64_t p) {
  return p < a.M && a.ev[p] >= 0 && a.parent[p] == (int32_t)p && a.sz[p] >= a.d.min_size;
}

// A workgroup owns CL_SPAN consecutive list positions, each of its 4 waves a contiguous quarter: ballot bit order == list order.
__device__ __forceinline__ int cl_wave_ballots(const ClArgs& a, int64_t p0, int lane, unsigned long long (&m)[CL_ITER]) {
  int c = 0;
#pragma unroll
  for (int t = 0; t < CL_ITER; ++t) {
    m[t] = __ballot(cl_kept_rep(a, p0 + t * 64 + lane));
    c += __popcll(m[t]);
  }
  return c;
}

__global__ __launch_bounds__(256) void cluster_count_kernel(ClArgs a) {
  __shared__ int sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long m[CL_ITER];
  const int c = cl_wave_ballots(a, (int64_t)blockIdx.x * CL_SPAN + wave * (64 * CL_ITER), lane, m);
  if (lane == 0) sm[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// ONE workgroup turns the counts into exclusive prefixes in place, in list order: a thread's chunk serially, lanes by shuffles, waves
// through LDS in wave order.
__global__ __launch_bounds__(1024) void cluster_scan_kernel(int32_t* __restrict__ cnt, int64_t B, int32_t* __restrict__ total_out) {
  __shared__ int wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = (B + 1023) / 1024;
  int64_t lo = threadIdx.x * chunk, hi = lo + chunk;
  if (lo > B) lo = B;
  if (hi > B) hi = B;
  int s = 0;
  for (int64_t i = lo; i < hi; ++i) s += cnt[i];
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
    const int t = cnt[i];
    cnt[i] = excl;
    excl += t;
  }
  if (threadIdx.x == 0) *total_out = total;
}

// rank[p] = kept representatives at positions < p, for every p < M
__global__ __launch_bounds__(256) void cluster_rank_kernel(ClArgs a) {
  __shared__ int sm[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * CL_SPAN + wave * (64 * CL_ITER);
  unsigned long long m[CL_ITER];
  const int c = cl_wave_ballots(a, p0, lane, m);
  if (lane == 0) sm[wave] = c;
  __syncthreads();
  int pos = a.cnt[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos += sm[w];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int t = 0; t < CL_ITER; ++t) {
    const int64_t p = p0 + t * 64 + lane;
    if (p < a.M) a.rank[p] = pos + __popcll(m[t] & below);
    pos += __popcll(m[t]);
  }
}

__device__ __forceinline__ int32_t cl_rank_at(const ClArgs& a, int64_t p) { return a.M == 0 ? 0 : p < a.M ? a.rank[p] : *a.total; }

// Thread j < M: the entry's id and, at a kept representative, its table row.  Thread t <= n: the event's count and table offset.
__global__ __launch_bounds__(256) void cluster_output_kernel(ClArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < a.M) {
    const int e = a.ev[j];
    int32_t id = -1;
    if (e >= 0) {
      const int32_t r = a.parent[j];
      if (a.sz[r] >= a.d.min_size) {
        const int64_t lo = cl_clamp(a.d.offsets[e], a.M);
        const int32_t row = a.rank[r];
        id = row - cl_rank_at(a, lo);
        if (r == (int32_t)j && row < a.o.cap) {
          if (a.o.first) a.o.first[row] = (int32_t)(j - lo);
          if (a.o.size) a.o.size[row] = a.sz[r];
          if (a.o.cls) a.o.cls[row] = a.d.cls[j];
        }
      }
    }
    a.o.cluster[j] = id;
  }
  if (j <= a.d.n) {
    if (j < a.d.n) {
      const int64_t lo = cl_clamp(a.d.offsets[j], a.M);
      int64_t hi = cl_clamp(a.d.offsets[j + 1], a.M);
      if (hi < lo) hi = lo;
      const int32_t rl = cl_rank_at(a, lo);
      a.o.count[j] = cl_rank_at(a, hi) - rl;
      if (a.o.table_offsets) a.o.table_offsets[j] = rl;
    } else if (a.o.table_offsets) {
      a.o.table_offsets[j] = cl_rank_at(a, a.M);
    }
    if (a.M == 0 && j == 0) *a.o.status = 0;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline int64_t cl_blocks(int64_t m) { return cdiv64(m, CL_SPAN); }

extern "C" size_t ursn_cluster_scratch_bytes(int32_t n, int64_t m_total) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 31)) return 0;
  const size_t words = 4 * (size_t)m_total + (size_t)cl_blocks(m_total) + 2;
  return (words * sizeof(int32_t) + 7) & ~(size_t)7;
}

extern "C" int ursn_cluster_voxels(const ursn_cluster_desc* d, const ursn_cluster_out* out, void* scratch, size_t scratch_bytes,
                                   void* stream) {
  const char* who = "cluster_voxels";
  URSN_REQUIRE(d && out, "%s: null desc / out", who);
  URSN_REQUIRE(d->ndim == 2 || d->ndim == 3, "%s: ndim = %d, must be 2 or 3", who, (int)d->ndim);
  int64_t vox = 1;
  for (int i = 0; i < d->ndim; ++i) {
    URSN_REQUIRE(d->spatial[i] >= 1, "%s: spatial[%d] = %d < 1", who, i, (int)d->spatial[i]);
    vox *= d->spatial[i];
    URSN_REQUIRE(vox < ((int64_t)1 << 31), "%s: prod(spatial) >= 2^31 (indices are int32)", who);
  }
  const int c = d->connectivity;
  URSN_REQUIRE(d->ndim == 3 ? (c == 6 || c == 18 || c == 26) : (c == 4 || c == 8),
               "%s: connectivity = %d, must be 6, 18 or 26 in 3-D and 4 or 8 in 2-D", who, c);
  URSN_REQUIRE(d->same_class == 0 || d->same_class == 1, "%s: same_class = %d, must be 0 or 1", who, (int)d->same_class);
  URSN_REQUIRE(d->min_size >= 1, "%s: min_size = %d < 1", who, (int)d->min_size);
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)d->n);
  URSN_REQUIRE(d->m_total >= 0 && d->m_total < ((int64_t)1 << 31), "%s: m_total = %lld outside [0, 2^31)", who,
               (long long)d->m_total);
  URSN_REQUIRE(d->offsets, "%s: null offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cls), "%s: null index / cls", who);
  URSN_REQUIRE(d->m_total == 0 || out->cluster, "%s: null out->cluster", who);
  URSN_REQUIRE(out->count && out->status, "%s: null out->count / out->status", who);
  URSN_REQUIRE(out->cap >= 0, "%s: cap = %lld < 0", who, (long long)out->cap);
  URSN_REQUIRE(!(out->first || out->size || out->cls) || out->table_offsets, "%s: a table array needs table_offsets", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)out->table_offsets | (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)out->cluster | (uintptr_t)out->count | (uintptr_t)out->first | (uintptr_t)out->size |
                 (uintptr_t)out->status) & 3) == 0,
               "%s: index / cluster / count / first / size / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_scratch_bytes(d->n, d->m_total);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  ClArgs a;
  a.d = *d;
  a.o = *out;
  if (d->ndim == 3) a.S[0] = d->spatial[0], a.S[1] = d->spatial[1], a.S[2] = d->spatial[2];
  else a.S[0] = 1, a.S[1] = d->spatial[0], a.S[2] = d->spatial[1];
  a.maxax = d->ndim == 3 ? (c == 6 ? 1 : c == 18 ? 2 : 3) : (c == 4 ? 1 : 2);
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.B = cl_blocks(M);
  a.parent = (int32_t*)scratch;
  a.sz = a.parent + M;
  a.ev = a.sz + M;
  a.rank = a.ev + M;
  a.cnt = a.rank + M;
  a.total = a.cnt + a.B;
  hipStream_t s = (hipStream_t)stream;
  const dim3 per_entry((unsigned)cdiv64(M, 256));
  if (M > 0) {
    ursn_note_kernel("cluster_init");
    hipLaunchKernelGGL(cluster_init_kernel, per_entry, dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("cluster_merge");
    hipLaunchKernelGGL(cluster_merge_kernel, dim3((unsigned)cdiv64(4 * M, 256)), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("cluster_flatten");
    hipLaunchKernelGGL(cluster_flatten_kernel, per_entry, dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("cluster_count");
    hipLaunchKernelGGL(cluster_count_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("cluster_scan");
    hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(1024), 0, s, a.cnt, a.B, a.total);
    URSN_HIP(hipGetLastError());
    ursn_note_kernel("cluster_rank");
    hipLaunchKernelGGL(cluster_rank_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    URSN_HIP(hipGetLastError());
  }
  const int64_t threads = M > (int64_t)d->n + 1 ? M : (int64_t)d->n + 1;
  ursn_note_kernel("cluster_output");
  hipLaunchKernelGGL(cluster_output_kernel, dim3((unsigned)cdiv64(threads, 256)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
