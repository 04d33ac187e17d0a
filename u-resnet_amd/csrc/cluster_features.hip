// Per-cluster object records (gfx950): ursn_cluster_features reduces the members of every cluster ursn_cluster_voxels numbered to
// one row of an int64 table (count, charge, coordinate sums, box, anchored second moments, end points) and one row of an fp64 table
// (centroid, covariance, eigenvalues, principal axis, length).  include/uresnet_hip.h names the columns; uresnet_amd/clusters.py
// (cluster_features_numpy, jacobi_eigen3) states every field operation by operation, and this file follows it: the same bits.
//
// Why integers.  A cluster's members are scattered over workgroups, so the sums are accumulated with global atomics, and an atomic
// sum arrives in any order.  Every accumulated quantity is therefore a 64-bit INTEGER (add / min / max, agent scope): coordinates are
// integers already, the charge is summed in fixed point (rint(value * 2^16)), and the second moments are taken around an integer
// anchor (the centroid rounded to a voxel), which also removes the cancellation of E[x^2] - E[x]^2: |sum(x - m) / n| <= 0.5.
// Bounds with every extent <= 32768 and fewer than 2^31 entries: |s|, |d| < 2^15 * 2^31 = 2^46; |dd| < 2^30 * 2^31 = 2^61;
// |rint(value * 2^16)| <= 2^31 for |value| < 2^15, so |charge| <= 2^62.  No float atomics.  The end points are found with one 64-bit
// atomic min / max each on (order-preserving code of the fp32 projection) << 32 | position (max: the complemented position), so
// equal projections fall to the lower list position at both ends.  Everything in fp64 is computed per cluster by ONE thread in a
// fixed order under contract(off); fp64 divide and sqrt are correctly rounded on this device.
//
// Contention.  Neighbouring list entries very often share a cluster.  Before anything reaches global memory the lanes of a wave that
// hold the same row next to each other are combined by a segmented shuffle reduction, the first lane of each run adds the run to a
// 256-slot table of the workgroup in LDS (open addressing on the row; at most 256 runs per workgroup, so it cannot fill up and a
// probe walk is capped at 256 slots; 64-bit integer LDS atomics), and each distinct row of the workgroup then costs ONE global atomic
// per field (integer sums, minima and maxima: exact, whatever the grouping).  The second step is what a dense list needs, where two
// or three giant clusters alternate from lane to lane and wave runs are short.  URSN_CLFEAT_WAVE=0 keeps one global atomic per
// entry and field, the plain route the bits are compared against.
//
// Launches: init (rows below the device-read count, status), first-order + box pass (also stores every entry's row in the scratch),
// anchor + centroid per row, second-order pass, covariance + Jacobi + axis per row, projection pass, end points + length per row.
// Per-entry grids are sized by m_total; per-row kernels stride up to min(table_offsets[n], cap, m_total).  Every loop is bounded: the
// event search runs at most 17 halvings, the Jacobi schedule is fixed, the strides end at the count.
#include "ursn_common.h"

#pragma clang fp contract(off)

#define CF_I URSN_CLFEAT_I
#define CF_R URSN_CLFEAT_R
enum { CF_N = 0, CF_CHARGE = 1, CF_S = 2, CF_LO = 5, CF_HI = 8, CF_M = 11, CF_D = 14, CF_DD = 17, CF_FLAGS = 23, CF_ELO = 24, CF_EHI = 25 };
enum { CR_CENT = 0, CR_COV = 3, CR_EVAL = 9, CR_AXIS = 12, CR_LEN = 15, CR_TLO = 16, CR_THI = 17 };
#define CF_ROW_BLOCKS 1024   // workgroup cap of the per-row kernels (they stride)

struct CfArgs {
  ursn_cluster_feat_desc d;
  ursn_cluster_feat_out o;
  int S[3];          // the shape as three axes, last fastest; the coordinates of a 2-D shape are (x0, x1, 0)
  int32_t M;         // == d.m_total
  int64_t rows_max;  // min(cap, m_total): no more rows can have a member
  int32_t* row;      // [M] scratch: table row of the entry, -1 = skipped
  int combine;       // 1: equal-row lanes of a wave share one atomic
};

typedef long long cf_i64;
typedef unsigned long long cf_u64;

__device__ __forceinline__ void cf_add(int64_t* p, cf_i64 v) {
  __hip_atomic_fetch_add((cf_i64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cf_min(int64_t* p, cf_i64 v) {
  __hip_atomic_fetch_min((cf_i64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cf_max(int64_t* p, cf_i64 v) {
  __hip_atomic_fetch_max((cf_i64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cf_umin(int64_t* p, cf_u64 v) {
  __hip_atomic_fetch_min((cf_u64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cf_umax(int64_t* p, cf_u64 v) {
  __hip_atomic_fetch_max((cf_u64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows the per-row kernels walk: the device-read cluster count, never more than the table holds or the list could fill.
__device__ __forceinline__ int64_t cf_rows(const CfArgs& a) {
  const int64_t k = a.d.table_offsets[a.d.n];
  return k < 0 ? 0 : k > a.rows_max ? a.rows_max : k;
}

// A run = consecutive lanes of the wave with the same row >= 0.  Returns the lane one past the end of this lane's run and whether
// this lane is the run's first (it issues the atomics).  Without combining every active lane is its own run.
__device__ __forceinline__ int cf_run(int row, int lane, int combine, bool& lead) {
  const bool act = row >= 0;
  if (!combine) {
    lead = act;
    return lane + 1;
  }
  const int up = __shfl_up(row, 1, 64);
  const bool head = act && (lane == 0 || up != row);
  const cf_u64 mh = __ballot(head), ma = __ballot(act);
  const cf_u64 above = ~((2ull << lane) - 1ull);   // lanes above this one (lane 63: none)
  const cf_u64 nb = (mh | ~ma) & above;
  lead = head;
  return act ? (nb ? __ffsll((cf_i64)nb) - 1 : 64) : lane + 1;
}

// Segmented suffix reductions by doubling: after the step of distance d a lane holds its run's lanes [lane, min(lane + 2d, end)).
// Every lane of the wave calls them (the shuffles need all lanes); `combine` is uniform.
template <class T>
__device__ __forceinline__ T cf_seg_sum(T v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T o = __shfl_down(v, d, 64);
      if (lane + d < end) v += o;
    }
  }
  return v;
}
template <class T>
__device__ __forceinline__ T cf_seg_min(T v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T o = __shfl_down(v, d, 64);
      if (lane + d < end && o < v) v = o;
    }
  }
  return v;
}
template <class T>
__device__ __forceinline__ T cf_seg_max(T v, int lane, int end, int combine) {
  if (combine) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T o = __shfl_down(v, d, 64);
      if (lane + d < end && o > v) v = o;
    }
  }
  return v;
}

enum { OP_ADD = 0, OP_MIN = 1, OP_MAX = 2, OP_UMIN = 3, OP_UMAX = 4 };
__device__ __forceinline__ cf_i64 cf_identity(int op) {
  return op == OP_ADD ? 0 : op == OP_MIN ? INT64_MAX : op == OP_MAX ? INT64_MIN : op == OP_UMIN ? -1 : 0;
}
__device__ __forceinline__ void cf_global(int64_t* p, int op, cf_i64 v) {
  if (v == cf_identity(op)) return;
  if (op == OP_ADD) cf_add(p, v);
  else if (op == OP_MIN) cf_min(p, v);
  else if (op == OP_MAX) cf_max(p, v);
  else if (op == OP_UMIN) cf_umin(p, (cf_u64)v);
  else cf_umax(p, (cf_u64)v);
}
__device__ __forceinline__ void cf_local(cf_i64* p, int op, cf_i64 v) {   // p in LDS
  if (v == cf_identity(op)) return;
  if (op == OP_ADD) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else if (op == OP_MIN) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else if (op == OP_MAX) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else if (op == OP_UMIN) __hip_atomic_fetch_min((cf_u64*)p, (cf_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else __hip_atomic_fetch_max((cf_u64*)p, (cf_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The run totals v[0..NF) of the lead lanes (field f is combined by op[f] into column col[f] of the row) -> the int64 table.  With
// combining: through the workgroup's LDS table, one global atomic per distinct row and field; every thread of the workgroup calls
// this (two barriers; `combine` is uniform).  Without: straight to global memory.
template <int NF>
__device__ __forceinline__ void cf_commit(const CfArgs& a, int32_t* tkey, cf_i64* tval, const int (&op)[NF], const int (&col)[NF],
                                          int row, bool lead, const cf_i64 (&v)[NF]) {
  if (!a.combine) {
    if (lead) {
      int64_t* t = a.o.itab + (int64_t)row * CF_I;
#pragma unroll
      for (int f = 0; f < NF; ++f) cf_global(t + col[f], op[f], v[f]);
    }
    return;
  }
  tkey[threadIdx.x] = -1;
#pragma unroll
  for (int f = 0; f < NF; ++f) tval[threadIdx.x * NF + f] = cf_identity(op[f]);
  __syncthreads();
  if (lead) {
    uint32_t slot = ((uint32_t)row * 2654435761u) >> 24;
    bool placed = false;
    for (int probe = 0; probe < 256 && !placed; ++probe) {
      const int32_t old = atomicCAS(&tkey[slot], -1, row);
      if (old == -1 || old == row) placed = true;
      else slot = (slot + 1) & 255;
    }
    if (placed) {
#pragma unroll
      for (int f = 0; f < NF; ++f) cf_local(tval + slot * NF + f, op[f], v[f]);
    } else {   // cannot happen (at most 256 runs, 256 slots); the totals still arrive
      int64_t* t = a.o.itab + (int64_t)row * CF_I;
#pragma unroll
      for (int f = 0; f < NF; ++f) cf_global(t + col[f], op[f], v[f]);
    }
  }
  __syncthreads();
  const int32_t key = tkey[threadIdx.x];
  if (key >= 0) {
    int64_t* t = a.o.itab + (int64_t)key * CF_I;
#pragma unroll
    for (int f = 0; f < NF; ++f) cf_global(t + col[f], op[f], tval[threadIdx.x * NF + f]);
  }
}

__device__ __forceinline__ void cf_coords(const CfArgs& a, int32_t idx, int ndim, int (&x)[3]) {
  const uint32_t u = (uint32_t)idx, S1 = (uint32_t)a.S[1], S2 = (uint32_t)a.S[2];
  const uint32_t q = u / S2;
  const int c2 = (int)(u - q * S2), c1 = (int)(q % S1), c0 = (int)(q / S1);
  if (ndim == 3) x[0] = c0, x[1] = c1, x[2] = c2;
  else x[0] = c1, x[1] = c2, x[2] = 0;
}

// ---- launch 1: rows below the count, and the status word -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clfeat_init_kernel(CfArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t0 == 0) *a.o.status = 0;
  const int64_t cells = cf_rows(a) * CF_I, step = (int64_t)gridDim.x * 256;
  for (int64_t t = t0; t < cells; t += step) {
    const int c = (int)(t % CF_I);
    int64_t v = 0;
    if (c >= CF_LO && c < CF_LO + 3) v = INT64_MAX;
    else if (c >= CF_HI && c < CF_HI + 3) v = INT64_MIN;
    else if (c == CF_ELO) v = -1;   // all ones: the identity of the unsigned minimum
    a.o.itab[t] = v;
  }
}

// ---- launch 2: one thread per list entry: its row, then count, charge, sums and box ------------------------------------------------
__global__ __launch_bounds__(256) void clfeat_first_kernel(CfArgs a) {
  __shared__ int32_t tkey[256];
  __shared__ cf_i64 tval[256 * 12];
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int row = -1, x[3] = {0, 0, 0};
  cf_i64 q = 0;
  int bad = 0;
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
        *a.o.status = 1;           // not a list ursn_cluster_voxels labelled
      } else if (r < a.rows_max) {
        row = (int)r;
        cf_coords(a, idx, a.d.ndim, x);
        if (a.d.value) {
          const float v = a.d.value[j];
          if (fabsf(v) < 32768.f) q = (cf_i64)rint((double)v * 65536.0);
          else bad = 1;            // too large for the fixed point, infinite or NaN
        }
      }
    }
    a.row[j] = row;
  }
  bool lead;
  const int end = cf_run(row, lane, a.combine, lead);
  cf_i64 v[12];
  v[0] = a.combine ? end - lane : 1;
  v[1] = cf_seg_sum(q, lane, end, a.combine);
  v[2] = cf_seg_max(bad, lane, end, a.combine) ? 1 : INT64_MIN;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[3 + c] = cf_seg_sum(x[c], lane, end, a.combine);      // at most 64 * 32767: an int
    v[6 + c] = cf_seg_min(x[c], lane, end, a.combine);
    v[9 + c] = cf_seg_max(x[c], lane, end, a.combine);
  }
  const int op[12] = {OP_ADD, OP_ADD, OP_MAX, OP_ADD, OP_ADD, OP_ADD, OP_MIN, OP_MIN, OP_MIN, OP_MAX, OP_MAX, OP_MAX};
  const int col[12] = {CF_N, CF_CHARGE, CF_FLAGS, CF_S, CF_S + 1, CF_S + 2, CF_LO, CF_LO + 1, CF_LO + 2, CF_HI, CF_HI + 1, CF_HI + 2};
  cf_commit<12>(a, tkey, tval, op, col, row, lead, v);
}

// ---- launch 3: per row: anchor and centroid -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void clfeat_anchor_kernel(CfArgs a) {
  const int64_t K = cf_rows(a), step = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < K; r += step) {
    int64_t* t = a.o.itab + r * CF_I;
    double* f = a.o.rtab + r * CF_R;
    const int64_t n = t[CF_N];
    if (n <= 0) {                  // a row without members: not a table ursn_cluster_voxels wrote
      *a.o.status = 2;
      for (int c = 0; c < 3; ++c) t[CF_M + c] = 0, t[CF_LO + c] = 0, t[CF_HI + c] = 0, f[CR_CENT + c] = 0.0;
      continue;
    }
    const double fn = (double)n;
    for (int c = 0; c < 3; ++c) {
      const int64_t s = t[CF_S + c];
      t[CF_M + c] = (2 * s + n) / (2 * n);   // s >= 0: the quotient is the floor
      f[CR_CENT + c] = (double)s / fn;
    }
  }
}

// ---- launch 4: one thread per list entry: first and second moments around the row's anchor ------------------------------------------
__global__ __launch_bounds__(256) void clfeat_second_kernel(CfArgs a) {
  __shared__ int32_t tkey[256];
  __shared__ cf_i64 tval[256 * 9];
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int row = j64 < a.M ? a.row[j64] : -1;
  int dx[3] = {0, 0, 0};
  if (row >= 0) {
    int x[3];
    cf_coords(a, a.d.index[j64], a.d.ndim, x);
    const int64_t* t = a.o.itab + (int64_t)row * CF_I;
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[c] = x[c] - (int)t[CF_M + c];
  }
  bool lead;
  const int end = cf_run(row, lane, a.combine, lead);
  cf_i64 v[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = cf_seg_sum(dx[c], lane, end, a.combine);
  const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int k = 0; k < 6; ++k) v[3 + k] = cf_seg_sum((cf_i64)dx[pa[k]] * (cf_i64)dx[pb[k]], lane, end, a.combine);
  const int op[9] = {OP_ADD, OP_ADD, OP_ADD, OP_ADD, OP_ADD, OP_ADD, OP_ADD, OP_ADD, OP_ADD};
  const int col[9] = {CF_D, CF_D + 1, CF_D + 2, CF_DD, CF_DD + 1, CF_DD + 2, CF_DD + 3, CF_DD + 4, CF_DD + 5};
  cf_commit<9>(a, tkey, tval, op, col, row, lead, v);
}

// One rotation of the pair (p, q) of clusters.py's jacobi_eigen3, r the third index; m = {00, 11, 22, 01, 02, 12}.
__device__ __forceinline__ void cf_rotate(double (&m)[6], double (&v)[3][3], int p, int q, int pq, int rp, int rq) {
  const double apq = m[pq];
  if (apq == 0.0) return;
  const double theta = (m[q] - m[p]) / (2.0 * apq);
  const double root = sqrt(theta * theta + 1.0);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + root);
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double tau = s / (1.0 + c);
  const double h = t * apq;
  m[p] = m[p] - h;
  m[q] = m[q] + h;
  m[pq] = 0.0;
  double g = m[rp], f = m[rq];
  m[rp] = g - s * (f + tau * g);
  m[rq] = f + s * (g - tau * f);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g = v[k][p], f = v[k][q];
    v[k][p] = g - s * (f + tau * g);
    v[k][q] = f + s * (g - tau * f);
  }
}

// ---- launch 5: per row: covariance, eigenvalues, axis ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void clfeat_axis_kernel(CfArgs a) {
  const int64_t K = cf_rows(a), step = (int64_t)gridDim.x * 64;
  for (int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x; r < K; r += step) {
    const int64_t* t = a.o.itab + r * CF_I;
    double* f = a.o.rtab + r * CF_R;
    const int64_t n = t[CF_N];
    if (n <= 0) {
      for (int c = CR_COV; c < CF_R; ++c) f[c] = 0.0;
      continue;
    }
    const double fn = (double)n;
    double mean[3], m[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = (double)t[CF_D + c] / fn;
    const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double prod = mean[pa[k]] * mean[pb[k]];
      m[k] = (double)t[CF_DD + k] / fn - prod;
      f[CR_COV + k] = m[k];
    }
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 8; ++sweep) {
      cf_rotate(m, v, 0, 1, 3, 4, 5);   // r = 2: a_rp = a_02, a_rq = a_12
      cf_rotate(m, v, 0, 2, 4, 3, 5);   // r = 1: a_rp = a_01, a_rq = a_12
      cf_rotate(m, v, 1, 2, 5, 3, 4);   // r = 0: a_rp = a_01, a_rq = a_02
    }
    // descending, equal values keep the lower column first: a stable insertion sort of three
    int o0 = 0, o1 = 1, o2 = 2;
    if (m[o1] > m[o0]) { const int x = o0; o0 = o1; o1 = x; }
    if (m[o2] > m[o1]) {
      const int x = o1; o1 = o2; o2 = x;
      if (m[o1] > m[o0]) { const int y = o0; o0 = o1; o1 = y; }
    }
    f[CR_EVAL + 0] = m[o0], f[CR_EVAL + 1] = m[o1], f[CR_EVAL + 2] = m[o2];
    double ax[3] = {o0 == 0 ? v[0][0] : o0 == 1 ? v[0][1] : v[0][2], o0 == 0 ? v[1][0] : o0 == 1 ? v[1][1] : v[1][2],
                    o0 == 0 ? v[2][0] : o0 == 1 ? v[2][1] : v[2][2]};
    int big = 0;
    if (fabs(ax[1]) > fabs(ax[big])) big = 1;
    if (fabs(ax[2]) > fabs(big == 0 ? ax[0] : ax[1])) big = 2;
    const double lead = big == 0 ? ax[0] : big == 1 ? ax[1] : ax[2];
    if (lead < 0.0) ax[0] = -ax[0], ax[1] = -ax[1], ax[2] = -ax[2];
    f[CR_AXIS + 0] = ax[0], f[CR_AXIS + 1] = ax[1], f[CR_AXIS + 2] = ax[2];
  }
}

// fp32 -> a 32-bit code whose unsigned order is the order of the values (a zero of either sign is +0 before it gets here)
__device__ __forceinline__ uint32_t cf_code(float t) {
  const uint32_t u = __float_as_uint(t);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cf_decode(uint32_t c) { return __uint_as_float((c & 0x80000000u) ? (c & 0x7FFFFFFFu) : ~c); }

// ---- launch 6: one thread per list entry: its projection on the row's axis, into the two end-point words -------------------------------
__global__ __launch_bounds__(256) void clfeat_project_kernel(CfArgs a) {
  __shared__ int32_t tkey[256];
  __shared__ cf_i64 tval[256 * 2];
  const int64_t j64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int row = j64 < a.M ? a.row[j64] : -1;
  cf_u64 klo = ~0ull, khi = 0ull;
  if (row >= 0) {
    int x[3];
    cf_coords(a, a.d.index[j64], a.d.ndim, x);
    const int64_t* t = a.o.itab + (int64_t)row * CF_I;
    const double* f = a.o.rtab + (int64_t)row * CF_R;
    const double p0 = f[CR_AXIS + 0] * (double)(x[0] - (int)t[CF_M + 0]);
    const double p1 = f[CR_AXIS + 1] * (double)(x[1] - (int)t[CF_M + 1]);
    const double p2 = f[CR_AXIS + 2] * (double)(x[2] - (int)t[CF_M + 2]);
    float tf = (float)((p0 + p1) + p2);
    if (tf == 0.f) tf = 0.f;       // -0 -> +0
    const cf_u64 code = (cf_u64)cf_code(tf) << 32;
    const uint32_t pos = (uint32_t)j64;
    klo = code | pos;
    khi = code | (uint32_t)~pos;
  }
  bool lead;
  const int end = cf_run(row, lane, a.combine, lead);
  const cf_i64 v[2] = {(cf_i64)cf_seg_min(klo, lane, end, a.combine), (cf_i64)cf_seg_max(khi, lane, end, a.combine)};
  const int op[2] = {OP_UMIN, OP_UMAX}, col[2] = {CF_ELO, CF_EHI};
  cf_commit<2>(a, tkey, tval, op, col, row, lead, v);
}

// ---- launch 7: per row: the two end points, their projections, the length --------------------------------------------------------------
__global__ __launch_bounds__(256) void clfeat_ends_kernel(CfArgs a) {
  const int64_t K = cf_rows(a), step = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < K; r += step) {
    int64_t* t = a.o.itab + r * CF_I;
    double* f = a.o.rtab + r * CF_R;
    if (t[CF_N] <= 0) {
      t[CF_ELO] = 0, t[CF_EHI] = 0;
      continue;
    }
    const cf_u64 klo = (cf_u64)t[CF_ELO], khi = (cf_u64)t[CF_EHI];
    const double tlo = (double)cf_decode((uint32_t)(klo >> 32)), thi = (double)cf_decode((uint32_t)(khi >> 32));
    t[CF_ELO] = (int64_t)(uint32_t)klo;
    t[CF_EHI] = (int64_t)(uint32_t)~(uint32_t)khi;
    f[CR_TLO] = tlo, f[CR_THI] = thi;
    f[CR_LEN] = thi - tlo;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
extern "C" size_t ursn_cluster_features_scratch_bytes(int32_t n, int64_t m_total, int64_t cap) {
  if (n < 1 || n > 65535 || m_total < 0 || m_total >= ((int64_t)1 << 31) || cap < 0) return 0;
  return (((size_t)m_total * sizeof(int32_t) + 7) & ~(size_t)7) + 8;
}

extern "C" int ursn_cluster_features(const ursn_cluster_feat_desc* d, const ursn_cluster_feat_out* out, void* scratch,
                                     size_t scratch_bytes, void* stream) {
  const char* who = "cluster_features";
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
  URSN_REQUIRE(out->cap >= 0, "%s: cap = %lld < 0", who, (long long)out->cap);
  URSN_REQUIRE(d->offsets && d->table_offsets, "%s: null offsets / table_offsets", who);
  URSN_REQUIRE(d->m_total == 0 || (d->index && d->cluster), "%s: null index / cluster", who);
  URSN_REQUIRE(out->status, "%s: null out->status", who);
  URSN_REQUIRE(out->cap == 0 || (out->itab && out->rtab), "%s: null out->itab / out->rtab", who);
  URSN_REQUIRE(scratch, "%s: null scratch", who);
  URSN_REQUIRE((((uintptr_t)d->offsets | (uintptr_t)d->table_offsets | (uintptr_t)out->itab | (uintptr_t)out->rtab |
                 (uintptr_t)scratch) & 7) == 0,
               "%s: offsets / table_offsets / itab / rtab / scratch must be 8-byte aligned", who);
  URSN_REQUIRE((((uintptr_t)d->index | (uintptr_t)d->value | (uintptr_t)d->cluster | (uintptr_t)out->status) & 3) == 0,
               "%s: index / value / cluster / status must be 4-byte aligned", who);
  const size_t need = ursn_cluster_features_scratch_bytes(d->n, d->m_total, out->cap);
  URSN_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes is too small, %zu needed", who, scratch_bytes, need);

  CfArgs a;
  a.d = *d;
  a.o = *out;
  if (d->ndim == 3) a.S[0] = d->spatial[0], a.S[1] = d->spatial[1], a.S[2] = d->spatial[2];
  else a.S[0] = 1, a.S[1] = d->spatial[0], a.S[2] = d->spatial[1];
  const int64_t M = d->m_total;
  a.M = (int32_t)M;
  a.rows_max = out->cap < M ? out->cap : M;
  a.row = (int32_t*)scratch;
  a.combine = ursn_env_on("URSN_CLFEAT_WAVE") ? 1 : 0;   // read at every call: the two routes are compared in one process
  hipStream_t s = (hipStream_t)stream;
  const dim3 per_entry((unsigned)cdiv64(M, 256));
  const int64_t rb256 = cdiv64(a.rows_max, 256), rb64 = cdiv64(a.rows_max, 64);
  const dim3 rows256((unsigned)(rb256 < 1 ? 1 : rb256 > CF_ROW_BLOCKS ? CF_ROW_BLOCKS : rb256));
  const dim3 rows64((unsigned)(rb64 < 1 ? 1 : rb64 > 4 * CF_ROW_BLOCKS ? 4 * CF_ROW_BLOCKS : rb64));
  const int64_t ib = cdiv64(a.rows_max * CF_I, 256);
  ursn_note_kernel("clfeat_init");
  hipLaunchKernelGGL(clfeat_init_kernel, dim3((unsigned)(ib < 1 ? 1 : ib > 4 * CF_ROW_BLOCKS ? 4 * CF_ROW_BLOCKS : ib)), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  if (a.rows_max == 0) return 0;   // no entry can belong to a row the table holds
  ursn_note_kernel("clfeat_first");
  hipLaunchKernelGGL(clfeat_first_kernel, per_entry, dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clfeat_anchor");
  hipLaunchKernelGGL(clfeat_anchor_kernel, rows256, dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clfeat_second");
  hipLaunchKernelGGL(clfeat_second_kernel, per_entry, dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clfeat_axis");
  hipLaunchKernelGGL(clfeat_axis_kernel, rows64, dim3(64), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clfeat_project");
  hipLaunchKernelGGL(clfeat_project_kernel, per_entry, dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("clfeat_ends");
  hipLaunchKernelGGL(clfeat_ends_kernel, rows256, dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}
