// Loss weights made on the device from the label alone (gfx950): ursn_make_weights, definition in include/uresnet_hip.h.  A
// stateless op-level pass like weight_norm.hip: three launches on the caller's stream, no atomics, no workgroup waits on another,
// nothing read that the same call did not write (the scratch needs no initialisation), and the only reductions are integer
// counts, so the same arguments give the same bits.
//   1. mkw_cat: a workgroup owns one box tile of one event (blockIdx.x = tile, blockIdx.y = event), 64 rows of 64 voxels along
//      the contiguous axis: 8 x 8 x 64 in 3-D, 64 x 64 in 2-D.  Thread t owns MKW_RUN = 16 consecutive voxels of row t / 4.  The
//      fp32 labels become one byte per voxel (class 0..7, MKW_NONE for "no class" and for positions outside the volume); with a
//      radius the tile and its radius-wide halo sit in LDS as bytes (rows padded to a multiple of 4 so that a thread reads the
//      16 + 2r bytes it needs of a neighbour row as dwords).  The category bytes go to a map in the scratch, the per-category
//      counts of the tile (ballot + popcount per wave, the four waves through LDS) to partial[event][tile][16].
//   2. mkw_reduce: one workgroup per event sums the tile counts, writes counts_out and the event's 16-entry weight table
//      (entries past ncls are 0, so is an empty category's; MKW_NONE = 15 indexes a 0).
//   3. mkw_write: a workgroup owns a fixed span of 4096 consecutive voxels of one event; weight = table[map byte], 16 map bytes
//      per lane in, four 16-byte stores out, the split into scalar head / vector body taken from the ADDRESS like wnorm_span's.
#include "ursn_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define MKW_TX 64       // tile extent along the contiguous axis
#define MKW_ROWS 64     // rows per tile: 8 x 8 (3-D), 64 (2-D)
#define MKW_RUN 16      // consecutive voxels per thread
#define MKW_SPAN 4096   // voxels per workgroup of the write pass (= voxels of a full tile)
#define MKW_NONE 15     // map byte of a voxel without category; table[15] == 0
#define MKW_TAB 16      // table / partial entries per event / tile (ncls + 1 <= 9 used)

struct MkwGeom {
  int D, H, W;        // 2-D: D == 1
  int nbx, nby;       // tiles along x and y
  int64_t V;
  int ncls;
};

struct MkwScale {
  float s[9];
};

template <int ND>
struct MkwTile {
  static constexpr int TZ = ND == 3 ? 8 : 1;
  static constexpr int TY = ND == 3 ? 8 : 64;
};

static inline int64_t mkw_tiles(int ndim, const int32_t* sp) {
  if (ndim == 3) return cdiv64(sp[0], MkwTile<3>::TZ) * cdiv64(sp[1], MkwTile<3>::TY) * cdiv64(sp[2], MKW_TX);
  return cdiv64(sp[0], MkwTile<2>::TY) * cdiv64(sp[1], MKW_TX);
}

__device__ __forceinline__ uint32_t mkw_code(float l, float ncls) { return (l > -1.0f && l < ncls) ? (uint32_t)(int)l : (uint32_t)MKW_NONE; }
__device__ __forceinline__ uint32_t mkw_byte(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }
// a class that can make a boundary: 1..7
__device__ __forceinline__ bool mkw_fg(uint32_t c) { return ((c - 1u) & 0xffu) < 7u; }

// 16 bytes to / from an address of any alignment: one 16-byte access, four dwords, or bytes
__device__ __forceinline__ void mkw_store16(uint8_t* p, const uint32_t* w) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
    u32x4 v = {w[0], w[1], w[2], w[3]};
    *(u32x4*)p = v;
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ((uint32_t*)p)[i] = w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = (uint8_t)mkw_byte(w, i);
  }
}
__device__ __forceinline__ void mkw_load16(const uint8_t* p, uint32_t* w) {
  const uintptr_t a = (uintptr_t)p;
  if ((a & 15) == 0) {
    const u32x4 v = *(const u32x4*)p;
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = ((const uint32_t*)p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
  }
}

// launch 1
template <int R, int ND>
__global__ __launch_bounds__(256) void mkw_cat_kernel(const float* __restrict__ label, MkwGeom g, uint8_t* __restrict__ map,
                                                      uint32_t* __restrict__ partial) {
  constexpr int TZ = MkwTile<ND>::TZ, TY = MkwTile<ND>::TY;
  constexpr int RZ = ND == 3 ? R : 0;
  constexpr int HZ = TZ + 2 * RZ, HY = TY + 2 * R, HX = MKW_TX + 2 * R, HXP = (HX + 3) & ~3;
  constexpr int WORDS = (MKW_RUN + 2 * R + 3) / 4;
  static_assert((MKW_TX - MKW_RUN) + 4 * WORDS <= HXP, "a thread's dword reads stay inside the padded row");
  __shared__ __attribute__((aligned(16))) uint8_t sm[R ? HZ * HY * HXP : 16];
  __shared__ uint32_t hist[4][MKW_TAB];

  const int t = threadIdx.x;
  const int e = blockIdx.y, b = blockIdx.x;
  const int bxi = b % g.nbx, bq = b / g.nbx, byi = bq % g.nby, bzi = bq / g.nby;
  const int z0 = bzi * TZ, y0 = byi * TY, xb = bxi * MKW_TX;
  const int row = t >> 2, lz = row / TY, ly = row % TY, x0 = (t & 3) * MKW_RUN;
  const int gz = z0 + lz, gy = y0 + ly, gx = xb + x0;
  const float* L = label + (int64_t)e * g.V;
  const float ncls = (float)g.ncls;
  const int64_t f = ((int64_t)gz * g.H + gy) * g.W + gx;
  int nin = 0;   // voxels of the run inside the volume
  if (gz < g.D && gy < g.H && gx < g.W) nin = g.W - gx < MKW_RUN ? g.W - gx : MKW_RUN;

  uint32_t my[4] = {0, 0, 0, 0};
  if (nin == MKW_RUN && (((uintptr_t)(L + f)) & 15) == 0) {
    const f32x4* A = (const f32x4*)(L + f);
    f32x4 x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = A[q];
#pragma unroll
    for (int i = 0; i < MKW_RUN; ++i) my[i >> 2] |= mkw_code(x[i >> 2][i & 3], ncls) << (8 * (i & 3));
  } else {
#pragma unroll
    for (int i = 0; i < MKW_RUN; ++i) {
      const uint32_t c = i < nin ? mkw_code(L[f + i], ncls) : (uint32_t)MKW_NONE;
      my[i >> 2] |= c << (8 * (i & 3));
    }
  }

  uint32_t bnd = 0;   // bit i: voxel i of the run is a boundary voxel
  if (R > 0) {
    // the run itself (positions outside the volume as MKW_NONE), then the halo cells around the tile
    uint8_t* own = sm + ((lz + RZ) * HY + (ly + R)) * HXP + R + x0;
#pragma unroll
    for (int i = 0; i < MKW_RUN; ++i) own[i] = (uint8_t)mkw_byte(my, i);
    for (int c = t; c < HZ * HY * HX; c += 256) {
      const int hx = c % HX, q = c / HX, hy = q % HY, hz = q / HY;
      if (hx >= R && hx < R + MKW_TX && hy >= R && hy < R + TY && hz >= RZ && hz < RZ + TZ) continue;
      const int z = z0 + hz - RZ, y = y0 + hy - R, x = xb + hx - R;
      uint32_t code = MKW_NONE;
      if (z >= 0 && z < g.D && y >= 0 && y < g.H && x >= 0 && x < g.W) code = mkw_code(L[((int64_t)z * g.H + y) * g.W + x], ncls);
      sm[(hz * HY + hy) * HXP + hx] = (uint8_t)code;
    }
    __syncthreads();
    uint32_t fg = 0;
#pragma unroll
    for (int i = 0; i < MKW_RUN; ++i) fg |= (uint32_t)mkw_fg(mkw_byte(my, i)) << i;
    if (fg) {
      // neighbour rows (dz, dy); byte j of a row's window is the voxel at x = gx - R + j, so voxel i sees bytes i .. i + 2R.
      // The voxel itself carries its own class and never counts.
      for (int dz = 0; dz <= 2 * RZ; ++dz) {
        for (int dy = 0; dy <= 2 * R; ++dy) {
          const uint32_t* rp = (const uint32_t*)(sm + ((lz + dz) * HY + (ly + dy)) * HXP + x0);
          uint32_t w[WORDS];
#pragma unroll
          for (int k = 0; k < WORDS; ++k) w[k] = rp[k];
#pragma unroll
          for (int i = 0; i < MKW_RUN; ++i) {
            const uint32_t m = mkw_byte(my, i);
            bool hit = false;
#pragma unroll
            for (int j = i; j <= i + 2 * R; ++j) {
              const uint32_t c = mkw_byte(w, j);
              hit = hit || (mkw_fg(c) && c != m);
            }
            bnd |= (uint32_t)hit << i;
          }
          if ((bnd & fg) == fg) goto scanned;   // every foreground voxel of the run is decided
        }
      }
    scanned:
      bnd &= fg;
    }
  }

  // categories: the boundary category is ncls
  uint32_t cat[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) cat[q] = 0;
#pragma unroll
  for (int i = 0; i < MKW_RUN; ++i) {
    const uint32_t k = ((bnd >> i) & 1u) ? (uint32_t)g.ncls : mkw_byte(my, i);
    cat[i >> 2] |= k << (8 * (i & 3));
  }
  if (nin > 0) {
    uint8_t* M = map + (int64_t)e * g.V + f;
    if (nin == MKW_RUN) {
      mkw_store16(M, cat);
    } else {
#pragma unroll
      for (int i = 0; i < MKW_RUN; ++i)
        if (i < nin) M[i] = (uint8_t)mkw_byte(cat, i);
    }
  }

  // per-wave histogram: positions outside the volume carry MKW_NONE and are counted nowhere
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    uint32_t cnt = 0;
    if (k <= g.ncls) {
#pragma unroll
      for (int i = 0; i < MKW_RUN; ++i) cnt += (uint32_t)__popcll(__ballot(mkw_byte(cat, i) == (uint32_t)k));
    }
    if (lane == 0) hist[wave][k] = cnt;
  }
  __syncthreads();
  if (t < MKW_TAB) {
    uint32_t v = 0;
    if (t < 9) v = (hist[0][t] + hist[1][t]) + (hist[2][t] + hist[3][t]);
    partial[((int64_t)e * gridDim.x + b) * MKW_TAB + t] = v;
  }
}

// launch 2: thread t sums entry t & 15 of tiles t >> 4, t >> 4 + 64, ...; the 64 groups meet through LDS
__global__ __launch_bounds__(1024) void mkw_reduce_kernel(const uint32_t* __restrict__ partial, int nb, int ncls, int mode, MkwScale sc,
                                                          int64_t* __restrict__ counts_out, float* __restrict__ table) {
  __shared__ uint32_t sm[64][MKW_TAB];
  const int t = threadIdx.x, k = t & 15, grp = t >> 4, e = blockIdx.x;
  const uint32_t* P = partial + (int64_t)e * nb * MKW_TAB + k;
  uint32_t acc = 0;   // a count never exceeds voxels < 2^31
  int bb = grp;
  for (; bb + 7 * 64 < nb; bb += 8 * 64) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = P[(int64_t)(bb + u * 64) * MKW_TAB];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; bb < nb; bb += 64) acc += P[(int64_t)bb * MKW_TAB];
  sm[grp][k] = acc;
  __syncthreads();
  if (t < MKW_TAB) {
    uint32_t total = 0;
    for (int q = 0; q < 64; ++q) total += sm[q][t];
    float w = 0.0f;
    if (t <= ncls) {
      if (counts_out) counts_out[(int64_t)e * (ncls + 1) + t] = (int64_t)total;
      if (total != 0) w = mode == URSN_WEIGHTS_INVFREQ ? (float)((double)sc.s[t] / (double)total) : sc.s[t];
    }
    table[(int64_t)e * MKW_TAB + t] = w;
  }
}

// launch 3
__global__ __launch_bounds__(256) void mkw_write_kernel(const uint8_t* __restrict__ map, const float* __restrict__ table, int64_t V,
                                                        float* __restrict__ out) {
  __shared__ float tab[MKW_TAB];
  const int t = threadIdx.x, e = blockIdx.y;
  const int64_t lo = (int64_t)blockIdx.x * MKW_SPAN;
  const int64_t left = V - lo;
  const int len = left < MKW_SPAN ? (int)left : MKW_SPAN;
  float* o = out + (int64_t)e * V + lo;
  const uint8_t* m = map + (int64_t)e * V + lo;
  if (t < MKW_TAB) tab[t] = table[(int64_t)e * MKW_TAB + t];
  __syncthreads();
  int h = (int)(((16 - ((uintptr_t)o & 15)) & 15) >> 2);
  if (h > len) h = len;
  if (t < h) o[t] = tab[m[t] & 15];
  const int i0 = h + MKW_RUN * t;
  if (i0 + MKW_RUN <= len) {
    uint32_t w[4];
    mkw_load16(m + i0, w);
    f32x4* O = (f32x4*)(o + i0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 y;
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = tab[mkw_byte(w, 4 * q + j) & 15];
      O[q] = y;
    }
  } else {
    for (int i = i0; i < len; ++i) o[i] = tab[m[i] & 15];
  }
}

static inline bool mkw_domain_ok(int32_t ndim, const int32_t* sp, int32_t n, int32_t ncls, int32_t radius, int64_t* voxels) {
  if ((ndim != 2 && ndim != 3) || !sp || n < 1 || n > 65535 || ncls < 1 || ncls > 8 || radius < 0 || radius > 3) return false;
  int64_t V = 1;
  for (int i = 0; i < ndim; ++i) {
    if (sp[i] < 1) return false;
    V *= sp[i];
    if (V >= ((int64_t)1 << 31)) return false;
  }
  *voxels = V;
  return true;
}

struct MkwScratch {
  size_t map, partial, table, total;   // byte offsets, then the size
};

static inline MkwScratch mkw_carve(int32_t ndim, const int32_t* sp, int32_t n, int64_t V) {
  MkwScratch s;
  s.map = 0;
  s.partial = ((size_t)n * (size_t)V + 15) & ~(size_t)15;
  s.table = s.partial + (size_t)n * (size_t)mkw_tiles(ndim, sp) * MKW_TAB * sizeof(uint32_t);
  s.total = s.table + (size_t)n * MKW_TAB * sizeof(float);
  return s;
}

extern "C" size_t ursn_make_weights_scratch_bytes(int32_t ndim, const int32_t* spatial, int32_t n, int32_t ncls, int32_t radius) {
  int64_t V = 0;
  if (!mkw_domain_ok(ndim, spatial, n, ncls, radius, &V)) return 0;
  return mkw_carve(ndim, spatial, n, V).total;
}

template <int R>
static void mkw_launch_cat(int ndim, dim3 grid, hipStream_t s, const float* label, const MkwGeom& g, uint8_t* map, uint32_t* partial) {
  if (ndim == 3)
    hipLaunchKernelGGL((mkw_cat_kernel<R, 3>), grid, dim3(256), 0, s, label, g, map, partial);
  else
    hipLaunchKernelGGL((mkw_cat_kernel<R, 2>), grid, dim3(256), 0, s, label, g, map, partial);
}

extern "C" int ursn_make_weights(const ursn_make_weights_desc* d, const float* label, float* weight_out, int64_t* counts_out,
                                 void* scratch, size_t scratch_bytes, void* stream) {
  URSN_REQUIRE(d && label && weight_out && scratch, "make_weights: null desc / label / weight_out / scratch");
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "make_weights: n = %d outside [1, 65535]", (int)d->n);
  URSN_REQUIRE(d->ndim == 2 || d->ndim == 3, "make_weights: ndim = %d, must be 2 or 3", (int)d->ndim);
  int64_t V = 1;
  for (int i = 0; i < d->ndim; ++i) {
    URSN_REQUIRE(d->spatial[i] >= 1, "make_weights: spatial[%d] = %d < 1", i, (int)d->spatial[i]);
    V *= d->spatial[i];
    URSN_REQUIRE(V < ((int64_t)1 << 31), "make_weights: prod(spatial) >= 2^31");
  }
  URSN_REQUIRE(V == d->voxels, "make_weights: prod(spatial) = %lld but voxels = %lld", (long long)V, (long long)d->voxels);
  URSN_REQUIRE(d->ncls >= 1 && d->ncls <= 8, "make_weights: ncls = %d outside [1, 8]", (int)d->ncls);
  URSN_REQUIRE(d->radius >= 0 && d->radius <= 3, "make_weights: radius = %d outside [0, 3]", (int)d->radius);
  URSN_REQUIRE(d->mode == URSN_WEIGHTS_CLASS || d->mode == URSN_WEIGHTS_INVFREQ, "make_weights: unknown mode %d", (int)d->mode);
  MkwScale sc;
  for (int k = 0; k < 9; ++k) sc.s[k] = 0.0f;
  for (int k = 0; k <= d->ncls; ++k) {
    URSN_REQUIRE(d->scale[k] - d->scale[k] == 0.0f, "make_weights: scale[%d] is not finite", k);
    sc.s[k] = d->scale[k];
  }
  URSN_REQUIRE((((uintptr_t)label | (uintptr_t)weight_out) & 3) == 0, "make_weights: label / weight_out must be 4-byte aligned");
  URSN_REQUIRE((((uintptr_t)scratch | (uintptr_t)counts_out) & 7) == 0, "make_weights: scratch / counts_out must be 8-byte aligned");
  const MkwScratch cv = mkw_carve(d->ndim, d->spatial, d->n, V);
  URSN_REQUIRE(scratch_bytes >= cv.total, "make_weights: scratch of %zu bytes is too small, %zu needed", scratch_bytes, cv.total);
  const uintptr_t la = (uintptr_t)label, wa = (uintptr_t)weight_out, bytes = (uintptr_t)d->n * (uintptr_t)V * sizeof(float);
  URSN_REQUIRE(la + bytes <= wa || wa + bytes <= la, "make_weights: weight_out overlaps label");

  hipStream_t s = (hipStream_t)stream;
  MkwGeom g;
  g.D = d->ndim == 3 ? d->spatial[0] : 1;
  g.H = d->ndim == 3 ? d->spatial[1] : d->spatial[0];
  g.W = d->ndim == 3 ? d->spatial[2] : d->spatial[1];
  g.nbx = (int)cdiv64(g.W, MKW_TX);
  g.nby = (int)cdiv64(g.H, d->ndim == 3 ? MkwTile<3>::TY : MkwTile<2>::TY);
  g.V = V;
  g.ncls = d->ncls;
  const int64_t nb = mkw_tiles(d->ndim, d->spatial);
  uint8_t* map = (uint8_t*)scratch + cv.map;
  uint32_t* partial = (uint32_t*)((char*)scratch + cv.partial);
  float* table = (float*)((char*)scratch + cv.table);
  const dim3 grid((unsigned)nb, (unsigned)d->n);
  ursn_note_kernel("mkw_cat");
  switch (d->radius) {
    case 0: mkw_launch_cat<0>(d->ndim, grid, s, label, g, map, partial); break;
    case 1: mkw_launch_cat<1>(d->ndim, grid, s, label, g, map, partial); break;
    case 2: mkw_launch_cat<2>(d->ndim, grid, s, label, g, map, partial); break;
    default: mkw_launch_cat<3>(d->ndim, grid, s, label, g, map, partial); break;
  }
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("mkw_reduce");
  hipLaunchKernelGGL(mkw_reduce_kernel, dim3((unsigned)d->n), dim3(1024), 0, s, (const uint32_t*)partial, (int)nb, (int)d->ncls,
                     (int)d->mode, sc, counts_out, table);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("mkw_write");
  hipLaunchKernelGGL(mkw_write_kernel, dim3((unsigned)cdiv64(V, MKW_SPAN), (unsigned)d->n), dim3(256), 0, s, (const uint8_t*)map,
                     (const float*)table, V, weight_out);
  URSN_HIP(hipGetLastError());
  return 0;
}
