// Cube-symmetry augmentation and test-time averaging at the boundary of the dense network (gfx950): ursn_sym_apply permutes the
// (data, label, weight) triple of a minibatch by one flip / axis-permutation code per event, ursn_sym_accumulate maps a score
// volume back and adds it to a running mean, ursn_voxels_to_dense_sym / ursn_voxel_index_sym do the same to a voxel list as index
// arithmetic inside the scatter the feed already runs.  Stateless op-level passes like those of voxel_io.hip and weight_norm.hip:
// HBM-bound, no atomics, no scratch, no workgroup waits on another, so the same arguments give the same bits.  The semantics
// (include/uresnet_hip.h): input voxel i lands at output voxel o with o[a] = f_a(i[P[a]]).
#include "ursn_common.h"

typedef uint32_t sym_u32x4 __attribute__((ext_vector_type(4)));

#define SYM_MAX_N 1024
#define SYM_T 32   // tile edge of the transposing path, in voxels

// ---- the codes (host and device) ---------------------------------------------------------------------------------------------
// Everything below works on the 3-D form of an op: a 2-D shape (H, W) is the 3-D shape (1, H, W) with axis 0 left alone.  An op
// byte is k * 8 + flips with k the index of P in lexicographic order and bit a of flips for output axis a; P[k] is packed two
// bits per axis, six bits per k, so that nothing is indexed dynamically (no scratch).
#define SYM_PERMS ((uint64_t)36 | (uint64_t)24 << 6 | (uint64_t)33 << 12 | (uint64_t)9 << 18 | (uint64_t)18 << 24 | (uint64_t)6 << 30)

__host__ __device__ __forceinline__ int sym_perm(int k, int a) { return (int)((SYM_PERMS >> (6 * k + 2 * a)) & 3); }
__host__ __device__ __forceinline__ int sym_sel3(int a, int x0, int x1, int x2) { return a == 0 ? x0 : a == 1 ? x1 : x2; }

static int sym_perm_index(int p0, int p1, int p2) {
  for (int k = 0; k < 6; ++k)
    if (sym_perm(k, 0) == p0 && sym_perm(k, 1) == p1 && sym_perm(k, 2) == p2) return k;
  return -1;
}

// code of `ndim` dimensions -> op byte of the 3-D form
static int sym_to3(int ndim, int code) { return ndim == 3 ? code : (code >> 2) * 8 + ((code & 3) << 1); }
static int sym_from3(int ndim, int op) { return ndim == 3 ? op : ((op >> 3) << 2) | ((op & 7) >> 1); }

extern "C" int ursn_sym_count(int32_t ndim) { return ndim == 3 ? 48 : ndim == 2 ? 8 : 0; }

extern "C" int ursn_sym_valid(int32_t ndim, const int32_t* spatial, int32_t code) {
  if (!spatial || code < 0 || code >= ursn_sym_count(ndim)) return 0;
  const int k = code >> ndim;   // 2-D: P = (0,1) | (1,0)
  for (int a = 0; a < ndim; ++a) {
    const int p = ndim == 3 ? sym_perm(k, a) : (k ? 1 - a : a);
    if (spatial[a] < 1 || spatial[p] != spatial[a]) return 0;
  }
  return 1;
}

extern "C" int ursn_sym_inverse(int32_t ndim, int32_t code) {
  if (code < 0 || code >= ursn_sym_count(ndim)) return -1;
  const int op = sym_to3(ndim, code), k = op >> 3, fl = op & 7;
  int inv[3], f = 0;
  for (int a = 0; a < 3; ++a) inv[sym_perm(k, a)] = a;
  for (int a = 0; a < 3; ++a) f |= ((fl >> inv[a]) & 1) << a;   // i[k] = f_{Pinv[k]}(o[Pinv[k]])
  return sym_from3(ndim, sym_perm_index(inv[0], inv[1], inv[2]) * 8 + f);
}

extern "C" int ursn_sym_compose(int32_t ndim, int32_t a, int32_t b) {
  const int cnt = ursn_sym_count(ndim);
  if (a < 0 || a >= cnt || b < 0 || b >= cnt) return -1;
  const int oa = sym_to3(ndim, a), ob = sym_to3(ndim, b);
  int p[3], f = 0;   // o[y] = fb_y(m[Pb[y]]), m[x] = fa_x(i[Pa[x]])
  for (int y = 0; y < 3; ++y) {
    const int x = sym_perm(ob >> 3, y);
    p[y] = sym_perm(oa >> 3, x);
    f |= ((((ob & 7) >> y) ^ ((oa & 7) >> x)) & 1) << y;
  }
  return sym_from3(ndim, sym_perm_index(p[0], p[1], p[2]) * 8 + f);
}

struct SymShape {
  int S0, S1, S2;   // the 3-D form of the shape
  int n;
  uint8_t ops[SYM_MAX_N];   // one op byte per event: the codes travel as launch arguments
};

// ndim / spatial / n / ops of every entry point: checked, then packed into the launch argument
static int sym_shape(const char* who, int32_t ndim, const int32_t* spatial, int32_t n, const int32_t* ops, SymShape* g,
                     int64_t* voxels) {
  URSN_REQUIRE(ndim == 2 || ndim == 3, "%s: ndim = %d not in {2, 3}", who, (int)ndim);
  URSN_REQUIRE(spatial && ops, "%s: null spatial / ops", who);
  URSN_REQUIRE(n >= 1 && n <= SYM_MAX_N, "%s: n = %d outside [1, %d] (the codes travel as launch arguments)", who, (int)n, SYM_MAX_N);
  int64_t V = 1;
  for (int a = 0; a < ndim; ++a) {
    URSN_REQUIRE(spatial[a] >= 1, "%s: spatial[%d] = %d < 1", who, a, (int)spatial[a]);
    V *= spatial[a];
    URSN_REQUIRE(V < ((int64_t)1 << 31), "%s: prod(spatial) >= 2^31", who);
  }
  for (int e = 0; e < n; ++e) {
    URSN_REQUIRE(ops[e] >= 0 && ops[e] < ursn_sym_count(ndim), "%s: ops[%d] = %d outside [0, %d)", who, e, (int)ops[e],
                 ursn_sym_count(ndim));
    URSN_REQUIRE(ursn_sym_valid(ndim, spatial, ops[e]), "%s: ops[%d] = %d permutes axes of unequal size", who, e, (int)ops[e]);
    g->ops[e] = (uint8_t)sym_to3(ndim, ops[e]);
  }
  g->S0 = ndim == 3 ? spatial[0] : 1, g->S1 = spatial[ndim - 2], g->S2 = spatial[ndim - 1], g->n = n;
  *voxels = V;
  return 0;
}

struct SymOp {
  int P0, P1, P2, fl;
};
__device__ __forceinline__ SymOp sym_decode(int op) {
  const int k = op >> 3;
  return SymOp{sym_perm(k, 0), sym_perm(k, 1), sym_perm(k, 2), op & 7};
}

// ---- ursn_sym_apply / ursn_sym_accumulate ------------------------------------------------------------------------------------
struct SymArgs {
  const uint32_t* src[3];
  uint32_t* dst[3];   // nullptr: pair not asked for
  int first;          // accumulate only
  float scale;
  SymShape g;
};

// what is stored for source bits v where the destination holds `*d` (read by ursn_sym_accumulate only, and not with `first`)
template <bool ACC>
__device__ __forceinline__ uint32_t sym_out(uint32_t v, const uint32_t* d, int first, float scale) {
  if constexpr (ACC) return __float_as_uint(((first ? 0.f : __uint_as_float(*d)) + __uint_as_float(v)) * scale);
  else return v;
}

// Source element of output element p of one event, for an op that keeps the last axis last (P2 == 2; P0, P1 is the identity
// or the swap of the two outer axes, which then have the same size).  L = S2 * C floats per row.
template <int C>
__device__ __forceinline__ int sym_row_src(int p, int L, const SymShape& g, const SymOp& o) {
  const int r = (int)((unsigned)p / (unsigned)L), x = p - r * L;
  const int o0 = (int)((unsigned)r / (unsigned)g.S1), o1 = r - o0 * g.S1;
  const int t0 = (o.fl & 1) ? g.S0 - 1 - o0 : o0, t1 = (o.fl & 2) ? g.S1 - 1 - o1 : o1;   // i[P[a]] = f_a(o[a])
  const int srow = o.P0 == 0 ? t0 * g.S1 + t1 : t1 * g.S1 + t0;
  if (!(o.fl & 4)) return srow * L + x;
  const int xv = x / C, c = x - xv * C;
  return srow * L + (g.S2 - 1 - xv) * C + c;
}

// blockIdx.y = event, blockIdx.z = tensor pair, blockIdx.x strides over the event's work.  The event's op picks the path for the
// whole workgroup.
//  * last axis stays last: the event's output is one flat array of `total` floats: `h` < 4 scalar elements up to the first
//    16-byte boundary, Q aligned float4s, < 4 scalar elements of tail (voxel_fill_kernel's split).  A float4 that lies inside
//    one row and whose source is four consecutive floats (no flip of the last axis, or C == 1: then reversed) is read with one
//    16-byte load when the source address is 16-byte aligned; everything else is read element by element.
//  * last axis moves: input axis q = P[2] becomes the output's last axis and the input's last axis becomes output axis a*.  A
//    workgroup transposes a tile of 32 (axis q) x 32 (last axis) voxels at a fixed index u of the third axis through LDS:
//    it reads 32 input rows of 32 * C contiguous floats and writes 32 output rows of 32 * C contiguous floats.  LDS row pitch
//    33 * C dwords: the stores run along a row (consecutive dwords), the loads of output lane l = rho * C + c read dword
//    rho * 33 C + jx * C + c = l + 32 C rho + jx C, which is l + const modulo the 32 banks a ds_read_b32 / ds_write_b32 lane
//    group of 32 sees: neither side has a bank conflict.  A flip of the output's last axis is taken at the LDS store (row
//    31 - jq), so the loads keep that pattern.
template <int C, bool ACC>
__global__ __launch_bounds__(256) void sym_kernel(SymArgs a) {
  __shared__ uint32_t tile[SYM_T * (SYM_T + 1) * C];
  const uint32_t* src = a.src[blockIdx.z];
  uint32_t* dst = a.dst[blockIdx.z];
  if (!dst) return;
  const SymShape& g = a.g;
  const SymOp o = sym_decode(g.ops[blockIdx.y]);
  const int L = g.S2 * C, total = g.S0 * g.S1 * L;
  src += (int64_t)blockIdx.y * total;
  dst += (int64_t)blockIdx.y * total;
  const int tid = threadIdx.x;

  if (o.P2 == 2) {
    int h = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
    if (h > total) h = total;
    const int Q = (total - h) >> 2;
    const bool rev = (o.fl & 4) != 0;
    for (int q = blockIdx.x * 256 + tid; q < Q; q += gridDim.x * 256) {
      const int p = h + 4 * q;
      const int x = (int)((unsigned)p % (unsigned)L);
      sym_u32x4 v;
      bool done = false;
      if (x + 4 <= L && (!rev || C == 1)) {
        const int s = sym_row_src<C>(rev ? p + 3 : p, L, g, o);   // lowest of the four source elements
        if ((((uintptr_t)(src + s)) & 15) == 0) {
          const sym_u32x4 w = *(const sym_u32x4*)(src + s);
          v = rev ? sym_u32x4{w[3], w[2], w[1], w[0]} : w;
        } else {
          v = rev ? sym_u32x4{src[s + 3], src[s + 2], src[s + 1], src[s]} : sym_u32x4{src[s], src[s + 1], src[s + 2], src[s + 3]};
        }
        done = true;
      }
      if (!done) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = src[sym_row_src<C>(p + j, L, g, o)];
      }
      sym_u32x4* O = (sym_u32x4*)(dst + p);
      if constexpr (ACC) {
        sym_u32x4 d = {0, 0, 0, 0};
        if (!a.first) d = *O;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t dj = d[j];
          v[j] = sym_out<true>(v[j], &dj, a.first, a.scale);
        }
      }
      *O = v;
    }
    if (blockIdx.x == 0 && tid < 6) {   // the < 4 head and < 4 tail elements
      const int p = tid < 3 ? tid : h + 4 * Q + (tid - 3);
      if (tid < 3 ? p < h : p < total) dst[p] = sym_out<ACC>(src[sym_row_src<C>(p, L, g, o)], dst + p, a.first, a.scale);
    }
    return;
  }

  const int q = o.P2;                      // input axis that becomes the output's last axis (0 | 1)
  const int astar = o.P0 == 2 ? 0 : 1;     // output axis that receives the input's last axis
  const int Sq = q == 0 ? g.S0 : g.S1, Sr = q == 0 ? g.S1 : g.S0;
  const int ntx = (g.S2 + SYM_T - 1) / SYM_T, ntq = (Sq + SYM_T - 1) / SYM_T;
  const int nt = Sr * ntq * ntx;
  const bool rev = (o.fl & 4) != 0;
  constexpr int ROW = SYM_T * C, PITCH = (SYM_T + 1) * C, ITER = SYM_T * ROW / 256;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const int tx = t % ntx, tmp = t / ntx;
    const int tq = tmp % ntq, u = tmp / ntq;
    const int x0 = tx * SYM_T, q0 = tq * SYM_T;
#pragma unroll
    for (int k = 0; k < ITER; ++k) {
      const int idx = tid + 256 * k;
      const int jq = idx / ROW, j = idx - jq * ROW;
      uint32_t v = 0;
      if (q0 + jq < Sq && x0 * C + j < L) {
        const int i0 = q == 0 ? q0 + jq : u, i1 = q == 0 ? u : q0 + jq;
        v = src[(i0 * g.S1 + i1) * L + x0 * C + j];
      }
      tile[(rev ? SYM_T - 1 - jq : jq) * PITCH + j] = v;
    }
    __syncthreads();
    const int o2lo = rev ? Sq - q0 - SYM_T : q0;   // Sq == S2: the op is valid
    const int ob_ = astar == 0 ? ((o.fl & 2) ? g.S1 - 1 - u : u) : ((o.fl & 1) ? g.S0 - 1 - u : u);
#pragma unroll
    for (int k = 0; k < ITER; ++k) {
      const int idx = tid + 256 * k;
      const int jx = idx / ROW, l = idx - jx * ROW;
      const int rho = l / C, c = l - rho * C;
      const int o2 = o2lo + rho;
      if (x0 + jx < g.S2 && o2 >= 0 && o2 < g.S2) {
        const int xi = x0 + jx;
        const int oa = astar == 0 ? ((o.fl & 1) ? g.S0 - 1 - xi : xi) : ((o.fl & 2) ? g.S1 - 1 - xi : xi);
        const int o0 = astar == 0 ? oa : ob_, o1 = astar == 0 ? ob_ : oa;
        uint32_t* d = dst + ((o0 * g.S1 + o1) * g.S2 + o2) * C + c;
        *d = sym_out<ACC>(tile[rho * PITCH + jx * C + c], d, a.first, a.scale);
      }
    }
    __syncthreads();
  }
}

static bool sym_overlap(const void* p, const void* q, uintptr_t bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + bytes && b < a + bytes;
}

template <bool ACC>
static int sym_launch(const char* who, const char* kname, const ursn_sym_desc* d, const float* const* src, float* const* dst,
                      int first, float scale, void* stream) {
  URSN_REQUIRE(d, "%s: null desc", who);
  SymArgs a;
  int64_t V = 0;
  URSN_TRY(sym_shape(who, d->ndim, d->spatial, d->n, d->ops, &a.g, &V));
  const int C = d->channels;
  URSN_REQUIRE(C >= 1 && C <= 8, "%s: channels = %d outside [1, 8]", who, C);
  URSN_REQUIRE(V * C < ((int64_t)1 << 31), "%s: prod(spatial) * channels = %lld >= 2^31", who, (long long)(V * C));
  URSN_REQUIRE(src[0] && dst[0], "%s: null first src / dst", who);
  const uintptr_t bytes = (uintptr_t)d->n * (uintptr_t)V * (uintptr_t)C * sizeof(float);
  for (int i = 0; i < 3; ++i) {
    URSN_REQUIRE((src[i] != nullptr) == (dst[i] != nullptr), "%s: src%d and dst%d must come together", who, i, i);
    URSN_REQUIRE((((uintptr_t)src[i] | (uintptr_t)dst[i]) & 3) == 0, "%s: src%d / dst%d must be 4-byte aligned", who, i, i);
    for (int j = 0; j < 3; ++j) {
      URSN_REQUIRE(!sym_overlap(dst[i], src[j], bytes), "%s: dst%d overlaps src%d (no in-place permutation)", who, i, j);
      URSN_REQUIRE(i == j || !sym_overlap(dst[i], dst[j], bytes), "%s: dst%d overlaps dst%d", who, i, j);
    }
    a.src[i] = (const uint32_t*)src[i], a.dst[i] = (uint32_t*)dst[i];
  }
  a.first = first, a.scale = scale;
  // blockIdx.x strides over an event's work: 4 float4 per thread for the row path, one tile per workgroup for the tile path
  int64_t gx = cdiv64(V * C, 4 * 256 * 4);
  for (int e = 0; e < d->n; ++e) {
    const int k = a.g.ops[e] >> 3, q = sym_perm(k, 2);
    if (q == 2) continue;
    const int64_t Sq = q == 0 ? a.g.S0 : a.g.S1, Sr = q == 0 ? a.g.S1 : a.g.S0;
    const int64_t nt = Sr * cdiv64(Sq, SYM_T) * cdiv64(a.g.S2, SYM_T);
    gx = nt > gx ? nt : gx;
  }
  gx = gx < 1 ? 1 : gx > (1 << 20) ? (1 << 20) : gx;
  const dim3 grid((unsigned)gx, (unsigned)d->n, dst[2] ? 3 : dst[1] ? 2 : 1);
  hipStream_t s = (hipStream_t)stream;
  ursn_note_kernel(kname);
  switch (C) {
#define SYM_CASE(c) case c: hipLaunchKernelGGL((sym_kernel<c, ACC>), grid, dim3(256), 0, s, a); break;
    SYM_CASE(1) SYM_CASE(2) SYM_CASE(3) SYM_CASE(4) SYM_CASE(5) SYM_CASE(6) SYM_CASE(7) SYM_CASE(8)
#undef SYM_CASE
  }
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_sym_apply(const ursn_sym_desc* d, const float* src0, float* dst0, const float* src1, float* dst1,
                              const float* src2, float* dst2, void* stream) {
  const float* src[3] = {src0, src1, src2};
  float* dst[3] = {dst0, dst1, dst2};
  return sym_launch<false>("sym_apply", "sym_apply", d, src, dst, 1, 1.f, stream);
}

extern "C" int ursn_sym_accumulate(const ursn_sym_desc* d, const float* src, float* dst, int32_t first, float scale, void* stream) {
  const float* s3[3] = {src, nullptr, nullptr};
  float* d3[3] = {dst, nullptr, nullptr};
  return sym_launch<true>("sym_accumulate", "sym_acc", d, s3, d3, first != 0, scale, stream);
}

// ---- ursn_voxels_to_dense_sym / ursn_voxel_index_sym -------------------------------------------------------------------------
// row-major index i of an event's voxel -> row-major index of its image o, o[a] = f_a(i[P[a]])
__device__ __forceinline__ int32_t sym_map_index(int32_t i, const SymShape& g, const SymOp& o) {
  const int i0 = i / (g.S1 * g.S2), r = i - i0 * (g.S1 * g.S2);
  const int i1 = r / g.S2, i2 = r - i1 * g.S2;
  int o0 = sym_sel3(o.P0, i0, i1, i2), o1 = sym_sel3(o.P1, i0, i1, i2), o2 = sym_sel3(o.P2, i0, i1, i2);
  if (o.fl & 1) o0 = g.S0 - 1 - o0;
  if (o.fl & 2) o1 = g.S1 - 1 - o1;
  if (o.fl & 4) o2 = g.S2 - 1 - o2;
  return (o0 * g.S1 + o1) * g.S2 + o2;
}

// voxel_scatter_kernel (voxel_io.hip) with the address taken through the event's op.  Indices are distinct inside an event and
// the op is a bijection of the event's voxels, so still no two threads share an address; an index outside [0, V) is skipped.
__global__ __launch_bounds__(256) void voxel_scatter_sym_kernel(ursn_voxel_batch b, SymShape g, float* __restrict__ data,
                                                                float* __restrict__ label, float* __restrict__ weight) {
  const int e = blockIdx.y;
  const SymOp o = sym_decode(g.ops[e]);
  int64_t lo = b.offsets[e];
  const int64_t hi = b.offsets[e + 1];
  if (lo < 0) lo = 0;
  const int64_t base = (int64_t)e * b.voxels;
  for (int64_t j = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; j < hi; j += (int64_t)gridDim.x * 256) {
    const int32_t i = b.index[j];
    if ((uint32_t)i >= (uint32_t)b.voxels) continue;
    const int64_t p = base + sym_map_index(i, g, o);
    data[p] = b.value[j];
    if (label) label[p] = b.label[j];
    if (weight) weight[p] = b.weight[j];
  }
}

__global__ __launch_bounds__(256) void voxel_index_sym_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ index,
                                                              int32_t* __restrict__ index_out, int64_t V, SymShape g) {
  const int e = blockIdx.y;
  const SymOp o = sym_decode(g.ops[e]);
  int64_t lo = offsets[e];
  const int64_t hi = offsets[e + 1];
  if (lo < 0) lo = 0;
  for (int64_t j = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; j < hi; j += (int64_t)gridDim.x * 256) {
    const int32_t i = index[j];
    index_out[j] = (uint32_t)i >= (uint32_t)V ? i : sym_map_index(i, g, o);
  }
}

extern "C" int ursn_voxels_to_dense_sym(const ursn_voxel_batch* b, int32_t ndim, const int32_t* spatial, const int32_t* ops,
                                        float* data, float* label, float* weight, void* stream) {
  URSN_REQUIRE(b && data, "voxels_to_dense_sym: null batch or data output");
  SymShape g;
  int64_t V = 0;
  URSN_TRY(sym_shape("voxels_to_dense_sym", ndim, spatial, b->n, ops, &g, &V));
  URSN_REQUIRE(V == b->voxels, "voxels_to_dense_sym: prod(spatial) = %lld, the batch has %lld voxels per event", (long long)V,
               (long long)b->voxels);
  hipStream_t s = (hipStream_t)stream;
  URSN_TRY(launch_voxel_fill(b, data, label, weight, s));   // ursn_voxels_to_dense's checks and its fill pass
  int64_t sx = cdiv64(b->voxels, 256 * 8);
  sx = sx < 1 ? 1 : sx > 1024 ? 1024 : sx;
  ursn_note_kernel("voxel_scatter_sym");
  hipLaunchKernelGGL(voxel_scatter_sym_kernel, dim3((unsigned)sx, (unsigned)b->n), dim3(256), 0, s, *b, g, data, label, weight);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_voxel_index_sym(int32_t ndim, const int32_t* spatial, int32_t n, const int32_t* ops, const int64_t* offsets,
                                    const int32_t* index, int32_t* index_out, void* stream) {
  SymShape g;
  int64_t V = 0;
  URSN_TRY(sym_shape("voxel_index_sym", ndim, spatial, n, ops, &g, &V));
  URSN_REQUIRE(offsets && index && index_out, "voxel_index_sym: null offsets / index / index_out");
  URSN_REQUIRE(((uintptr_t)offsets & 7) == 0 && (((uintptr_t)index | (uintptr_t)index_out) & 3) == 0,
               "voxel_index_sym: index / index_out must be 4-byte, offsets 8-byte aligned");
  URSN_REQUIRE(index != index_out, "voxel_index_sym: index_out must not be index (no in-place remap)");
  int64_t sx = cdiv64(V, 256 * 8);   // the list length lives on the device: sized like the scatter pass
  sx = sx < 1 ? 1 : sx > 1024 ? 1024 : sx;
  ursn_note_kernel("voxel_index_sym");
  hipLaunchKernelGGL(voxel_index_sym_kernel, dim3((unsigned)sx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, offsets, index,
                     index_out, V, g);
  URSN_HIP(hipGetLastError());
  return 0;
}
