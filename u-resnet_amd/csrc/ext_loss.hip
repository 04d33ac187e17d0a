// External loss boundary (gfx950): the three passes that open the network to a caller's own objective.
//   logits_dense      conv2's stored operands -> compact fp32 logits [n, voxels, ncls]          (ursn_logits_dense)
//   dlogits_pack      the caller's compact fp32 d(loss)/d(logits) -> the plan's dlog tensor      (ursn_dlogits_pack)
//   conv0_input_grad  conv0's stored dz and its weights -> d(loss)/d(input) [n, voxels, cin]      (ursn_conv0_input_grad)
// Stateless op-level passes like those of voxel_io.hip / weight_norm.hip: no atomics, no workgroup waits on another, nothing read
// that the same call did not get as an argument, so the same arguments give the same bits.  Where a pass must match another
// kernel's arithmetic (the logits of the heads, the dlogits the heads store, the BatchNorm-backward partials the heads carry) it
// RESTATES that kernel statement by statement, as vscores_kernel does: the heads are the benchmark's kernels and their generated
// code stays untouched.
#include "bf16_common.h"
#include "ext_loss.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

static int xl_check_dims(const char* who, int32_t n, int64_t voxels) {
  URSN_REQUIRE(n >= 1 && n <= 65535, "%s: n = %d outside [1, 65535]", who, (int)n);
  URSN_REQUIRE(voxels >= 1, "%s: voxels = %lld < 1", who, (long long)voxels);
  URSN_REQUIRE(voxels < ((int64_t)1 << 31), "%s: voxels = %lld >= 2^31", who, (long long)voxels);
  return 0;
}

// ---- logits_dense ----------------------------------------------------------------------------------------------------------
// The n events are one flat run of P = n * voxels voxels on both sides (z is [P][stride], the output [P][ncls] compact).  A
// workgroup owns a fixed span of XL_SPAN consecutive voxels: thread t loads voxels t, t + 256, ... (one 16-byte load each on the
// padded layouts), forms logit[k] = fmaf(raw[k], rstd[k], beta[k] - mean[k] * rstd[k]) exactly as the heads and vscores_kernel do,
// and leaves the span's len * ncls floats compact in LDS.  The span is then written as `h` < 4 scalar elements up to the first
// 16-byte boundary, Q aligned float4s and < 4 scalar elements of tail; the split is taken from the ADDRESS of the span (an output
// that is only 4-byte aligned moves it), and the LDS image is shifted by (4 - h) & 3 floats so the float4 reads are aligned too.
// A span is a multiple of 16 bytes for every ncls, so all full spans split alike.
#define XL_VPT 4
#define XL_SPAN (256 * XL_VPT)

struct LogitsArgs {
  ursn_vscores_desc d;
  float* out;
  int64_t P;
};

// MODE 0: fp32, any stride, scalar loads.  1: fp32, stride 4 | 8, 16-byte aligned z.  2: bf16 bit patterns, stride 8.
template <int MODE>
__global__ __launch_bounds__(256) void logits_dense_kernel(LogitsArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[XL_SPAN * 8 + 4];
  const ursn_vscores_desc& d = a.d;
  const int ncls = d.ncls, t = threadIdx.x;
  float sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sc[k] = 1.f;
    sh[k] = 0.f;
    if (k < ncls && d.mean) {
      sc[k] = d.rstd[k];
      sh[k] = d.beta[k] - d.mean[k] * sc[k];
    }
  }
  const int64_t nspans = (a.P + XL_SPAN - 1) / XL_SPAN;
  for (int64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
    const int64_t lo = sp * XL_SPAN;
    const int len = a.P - lo < XL_SPAN ? (int)(a.P - lo) : XL_SPAN;
    float raw[XL_VPT][8];
#pragma unroll
    for (int i = 0; i < XL_VPT; ++i) {   // every load of the span issued before the first use
      const int v = t + 256 * i;
#pragma unroll
      for (int k = 0; k < 8; ++k) raw[i][k] = 0.f;
      if (v < len) {
        const int64_t p = lo + v;
        if constexpr (MODE == 2) {
          unpack8(*(const u32x4*)((const bf16_t*)d.z + p * 8), raw[i]);
        } else if constexpr (MODE == 1) {
          const f32x4* zp = (const f32x4*)((const float*)d.z + p * d.z_cstride);
          const f32x4 z0 = zp[0];
#pragma unroll
          for (int k = 0; k < 4; ++k) raw[i][k] = z0[k];
          if (ncls > 4) {
            const f32x4 z1 = zp[1];
#pragma unroll
            for (int k = 0; k < 4; ++k) raw[i][4 + k] = z1[k];
          }
        } else {
          const float* zp = (const float*)d.z + p * d.z_cstride;
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (k < ncls) raw[i][k] = zp[k];
        }
      }
    }
    float* o = a.out + lo * ncls;
    const int total = len * ncls;
    int h = (int)(((16 - ((uintptr_t)o & 15)) & 15) >> 2);
    if (h > total) h = total;
    const int shift = (4 - h) & 3;   // element h of the span lands on a 16-byte boundary of the LDS image
#pragma unroll
    for (int i = 0; i < XL_VPT; ++i) {
      const int v = t + 256 * i;
      if (v < len) {
        float* l = lds + shift + v * ncls;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < ncls) l[k] = fmaf(raw[i][k], sc[k], sh[k]);
      }
    }
    __syncthreads();
    const int Q = (total - h) >> 2, tail = total - h - 4 * Q;
    if (Q > 0) {
      f32x4* O = (f32x4*)(o + h);
      const f32x4* L = (const f32x4*)(lds + shift + h);
      for (int q = t; q < Q; q += 256) O[q] = L[q];
    }
    if (t < h) o[t] = lds[shift + t];
    if (t < tail) o[h + 4 * Q + t] = lds[shift + h + 4 * Q + t];
    __syncthreads();
  }
}

int launch_logits_dense(const ursn_vscores_desc* d, float* logits_out, hipStream_t s) {
  URSN_REQUIRE(d && d->z && logits_out, "logits_dense: null desc / z / logits_out");
  URSN_TRY(xl_check_dims("logits_dense", d->n, d->voxels));
  URSN_REQUIRE(d->ncls >= 1 && d->ncls <= 8, "logits_dense: num_class %d not in [1,8]", (int)d->ncls);
  URSN_REQUIRE(d->dtype == 0 || d->dtype == 1, "logits_dense: dtype %d not in {0 fp32, 1 bf16}", (int)d->dtype);
  if (d->dtype == 1) {
    URSN_REQUIRE(d->z_cstride == 8, "logits_dense: bf16 z needs channel stride 8 (z_cstride = %d)", (int)d->z_cstride);
    URSN_REQUIRE(((uintptr_t)d->z & 15) == 0, "logits_dense: bf16 z must be 16-byte aligned");
  } else {
    URSN_REQUIRE(d->z_cstride >= d->ncls, "logits_dense: z_cstride %d < num_class %d", (int)d->z_cstride, (int)d->ncls);
    URSN_REQUIRE(((uintptr_t)d->z & 3) == 0, "logits_dense: fp32 z must be 4-byte aligned");
  }
  URSN_REQUIRE(!d->mean || (d->rstd && d->beta), "logits_dense: mean without rstd / beta");
  URSN_REQUIRE(((uintptr_t)logits_out & 3) == 0, "logits_dense: logits_out must be 4-byte aligned");
  LogitsArgs a;
  a.d = *d;
  a.out = logits_out;
  a.P = (int64_t)d->n * d->voxels;
  int64_t gx = cdiv64(a.P, XL_SPAN);
  gx = gx > ((int64_t)1 << 20) ? ((int64_t)1 << 20) : gx;
  ursn_note_kernel("logits_dense");
  if (d->dtype == 1) hipLaunchKernelGGL(logits_dense_kernel<2>, dim3((unsigned)gx), dim3(256), 0, s, a);
  else if ((d->z_cstride == 4 || d->z_cstride == 8) && ((uintptr_t)d->z & 15) == 0)
    hipLaunchKernelGGL(logits_dense_kernel<1>, dim3((unsigned)gx), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(logits_dense_kernel<0>, dim3((unsigned)gx), dim3(256), 0, s, a);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_logits_dense(const ursn_vscores_desc* d, float* logits_out, void* stream) {
  return launch_logits_dense(d, logits_out, (hipStream_t)stream);
}

// ---- dlogits_pack ----------------------------------------------------------------------------------------------------------
// One thread per voxel, grid-stride: p = block * 256 + thread, then + grid * 256 -- the partition of head_kernel / bhead_kernel,
// whose per-thread order of voxels this loop therefore shares (bhead_kernel takes two voxels per iteration, p and p + stride, in
// that order: the same sequence).  What is stored per voxel is what the head of the same layout stores:
//   fp32, stride 4, <= 4 classes : one 16-byte store {g[0..ncls), 0...}           (head_kernel's float4 branch)
//   fp32, any other stride       : the ncls values; the pad lanes are NOT written  (head_kernel's scalar branch; in a net they
//                                  hold the zeros ursn_create put there)
//   bf16, stride 8               : one 16-byte store of pack8({g[0..ncls), 0...}), round-to-nearest-even (bhead_kernel)
// BS: the BatchNorm-backward partials of the logits layer from the STORED values, restating the heads: per thread fp32 sums
// bg[k] += g, bgx[k] = fmaf(g, (z[k] - mean[k]) * rstd[k], bgx[k]) in voxel order, then per column the heads' tree over the 256
// threads in fp64; rows [block][3][C] with the third row zero (C = 4 fp32, 8 bf16): BnBwdArgs.pre_partial / BBnBwdArgs.pre_partial.
struct PackArgs {
  const float* g;
  int64_t P;
  int ncls;
  void* out;
  int ocs;
  const void* z;
  const float* mean;
  const float* rstd;
  double* bs;
};

template <int DT, bool V4, bool BS>
__global__ __launch_bounds__(256) void dlogits_pack_kernel(PackArgs a) {
  constexpr int C = DT == 1 ? 8 : 4;
  const int ncls = a.ncls;
  float bg[C], bgx[C], mu[C], sc[C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    bg[k] = bgx[k] = 0.f;
    mu[k] = 0.f;
    sc[k] = DT == 1 ? 0.f : 1.f;
    if (BS && k < ncls) { sc[k] = a.rstd[k]; mu[k] = a.mean[k]; }
  }
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.P; p += (int64_t)gridDim.x * blockDim.x) {
    const float* gp = a.g + p * ncls;
    if constexpr (DT == 1) {
      float d[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) d[k] = k < ncls ? gp[k] : 0.f;
      const u32x4 pk = pack8(d);
      *(u32x4*)((bf16_t*)a.out + p * 8) = pk;
      if constexpr (BS) {
        float dr[8], raw[8];
        unpack8(pk, dr);
        unpack8(*(const u32x4*)((const bf16_t*)a.z + p * 8), raw);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < ncls) { bg[k] += dr[k]; bgx[k] = fmaf(dr[k], (raw[k] - mu[k]) * sc[k], bgx[k]); }
      }
    } else if constexpr (V4) {
      f32x4 dv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < ncls) dv[k] = gp[k];
      *(f32x4*)((float*)a.out + p * 4) = dv;
      if constexpr (BS) {
        const f32x4 zv = *(const f32x4*)((const float*)a.z + p * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < ncls) { bg[k] += dv[k]; bgx[k] = fmaf(dv[k], (zv[k] - mu[k]) * sc[k], bgx[k]); }
      }
    } else {
      float* op = (float*)a.out + p * a.ocs;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) op[k] = gp[k];
    }
  }
  if constexpr (BS) {
    __shared__ double sm[4][256];
    constexpr int ROUNDS = 2 * C / 4;   // 2 C columns (sum g, sum g xhat) in rounds of four
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = 4 * r + k;
        sm[k][threadIdx.x] = col < C ? (double)bg[col % C] : (double)bgx[col % C];
      }
      __syncthreads();
      for (int st = 128; st >= 1; st >>= 1) {
        if (threadIdx.x < st)
          for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + st];
        __syncthreads();
      }
      if (threadIdx.x < 4) a.bs[(size_t)blockIdx.x * 3 * C + 4 * r + threadIdx.x] = sm[threadIdx.x][0];
    }
    if (threadIdx.x < C) a.bs[(size_t)blockIdx.x * 3 * C + 2 * C + threadIdx.x] = 0.0;
  }
}

int launch_dlogits_pack(const float* dlogits, int32_t n, int64_t voxels, int32_t ncls, void* out, int32_t out_cstride, int32_t dtype,
                        const void* z, const float* mean, const float* rstd, double* bs_partial, int bs_blocks, hipStream_t s) {
  URSN_REQUIRE(dlogits && out, "dlogits_pack: null dlogits / out");
  URSN_TRY(xl_check_dims("dlogits_pack", n, voxels));
  URSN_REQUIRE(ncls >= 1 && ncls <= 8, "dlogits_pack: num_class %d not in [1,8]", (int)ncls);
  URSN_REQUIRE(dtype == 0 || dtype == 1, "dlogits_pack: dtype %d not in {0 fp32, 1 bf16}", (int)dtype);
  URSN_REQUIRE(out_cstride >= ncls, "dlogits_pack: out_cstride %d < num_class %d", (int)out_cstride, (int)ncls);
  URSN_REQUIRE(((uintptr_t)dlogits & 3) == 0, "dlogits_pack: dlogits must be 4-byte aligned");
  if (dtype == 1) {
    URSN_REQUIRE(out_cstride == 8, "dlogits_pack: bf16 out needs channel stride 8 (out_cstride = %d)", (int)out_cstride);
    URSN_REQUIRE(((uintptr_t)out & 15) == 0, "dlogits_pack: bf16 out must be 16-byte aligned");
  } else {
    URSN_REQUIRE(((uintptr_t)out & 3) == 0, "dlogits_pack: fp32 out must be 4-byte aligned");
  }
  const bool v4 = dtype == 0 && out_cstride == 4 && ncls <= 4 && ((uintptr_t)out & 15) == 0;
  if (bs_partial) {
    URSN_REQUIRE(z && mean && rstd, "dlogits_pack: the BatchNorm-backward partials need z / mean / rstd");
    URSN_REQUIRE(((uintptr_t)z & 15) == 0 && ((uintptr_t)bs_partial & 7) == 0, "dlogits_pack: z must be 16-byte, the partials 8-byte aligned");
    URSN_REQUIRE(dtype == 1 || v4, "dlogits_pack: fp32 partials need the 4-padded layout (stride 4, <= 4 classes, 16-byte aligned)");
    URSN_REQUIRE(bs_blocks >= 1 && bs_blocks <= 16384, "dlogits_pack: %d partial blocks outside [1, 16384]", bs_blocks);
  }
  PackArgs a;
  a.g = dlogits; a.P = (int64_t)n * voxels; a.ncls = ncls; a.out = out; a.ocs = out_cstride;
  a.z = z; a.mean = mean; a.rstd = rstd; a.bs = bs_partial;
  int64_t gx = bs_partial ? bs_blocks : cdiv64(a.P, 256 * 4);
  gx = gx < 1 ? 1 : gx > 4096 && !bs_partial ? 4096 : gx;
  const dim3 grid((unsigned)gx), blk(256);
  ursn_note_kernel("dlogits_pack");
  if (dtype == 1) {
    if (bs_partial) hipLaunchKernelGGL((dlogits_pack_kernel<1, false, true>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((dlogits_pack_kernel<1, false, false>), grid, blk, 0, s, a);
  } else if (v4) {
    if (bs_partial) hipLaunchKernelGGL((dlogits_pack_kernel<0, true, true>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((dlogits_pack_kernel<0, true, false>), grid, blk, 0, s, a);
  } else {
    hipLaunchKernelGGL((dlogits_pack_kernel<0, false, false>), grid, blk, 0, s, a);
  }
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_dlogits_pack(const float* dlogits, int32_t n, int64_t voxels, int32_t ncls, void* out, int32_t out_cstride,
                                 int32_t dtype, void* stream) {
  return launch_dlogits_pack(dlogits, n, voxels, ncls, out, out_cstride, dtype, nullptr, nullptr, nullptr, nullptr, 0,
                             (hipStream_t)stream);
}

// ---- conv0_input_grad ------------------------------------------------------------------------------------------------------
// dinput[n, p, c] = sum over the 3^d taps k and the F channels f of dz[n, p - (k - 1), f] * w[k, c, f], SAME zero padding (the
// adjoint of conv0's forward z[p] = sum_k x[p + k - 1] w[k]).  A workgroup owns a tile of 4 x 4 x 16 voxels (3-D; 16 x 16 in
// 2-D), one voxel per thread, 64-byte runs along the fastest axis.  Per block of 8 channels the dz tile WITH its halo
// (6 x 6 x 18 | 18 x 18 voxels) is staged once into LDS as two planes of float4s (channels 0-3 | 4-7 of the block: a lane reads
// 16 bytes at a 16-byte lane stride), bf16 widened on the way; the block's weights [tap][CB][8] are staged beside it, rounded to
// bf16 on load on the bf16 plan (the value the plan's other data gradients use), and read as broadcasts.  No neighbour is read
// from global memory twice by one workgroup; accumulation is fp32 in tap order, channel order.
template <int ND> struct C0Tile;
template <> struct C0Tile<3> { static constexpr int TZ = 4, TY = 4, TX = 16, HZ = 6, NT = 27; };
template <> struct C0Tile<2> { static constexpr int TZ = 1, TY = 16, TX = 16, HZ = 1, NT = 9; };

struct C0Args {
  const void* dz;
  const float* w;
  float* out;
  int D0, D1, D2;     // spatial extents, D2 fastest (2-D: D0 = 1)
  int nty, ntx;       // tiles along D1 / D2
  int cin, F, dzcs;
  int vec;            // fp32: dz is 16-byte aligned with a stride that is a multiple of 4 floats: 16-byte loads
};

template <int ND, int DT, int CB>
__global__ __launch_bounds__(256) void conv0_input_grad_kernel(C0Args a) {
  using T = C0Tile<ND>;
  constexpr int TZ = T::TZ, TY = T::TY, TX = T::TX, HZ = T::HZ, HY = TY + 2, HX = TX + 2, NH = HZ * HY * HX, NT = T::NT;
  __shared__ f32x4 tile[2][NH];
  __shared__ __attribute__((aligned(16))) float wl[NT * CB * 8];
  const int t = threadIdx.x;
  const int tile_i = blockIdx.x;
  const int x0 = (tile_i % a.ntx) * TX, y0 = ((tile_i / a.ntx) % a.nty) * TY, z0 = (tile_i / (a.ntx * a.nty)) * TZ;
  const int lx = t % TX, ly = (t / TX) % TY, lz = t / (TX * TY);
  const int64_t V = (int64_t)a.D0 * a.D1 * a.D2;
  const int64_t img = (int64_t)blockIdx.y * V;
  const int gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
  const bool inside = gz < a.D0 && gy < a.D1 && gx < a.D2;
  for (int c0 = 0; c0 < a.cin; c0 += CB) {
    float acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[cb] = 0.f;
    for (int f0 = 0; f0 < a.F; f0 += 8) {
      __syncthreads();   // the previous block's reads of the two LDS images are done
      for (int i = t; i < NT * CB * 8; i += 256) {
        const int f = f0 + (i & 7), c = c0 + (i >> 3) % CB, tap = i / (8 * CB);
        float v = (c < a.cin && f < a.F) ? a.w[((int64_t)tap * a.cin + c) * a.F + f] : 0.f;
        if constexpr (DT == 1) v = bf2f(f2bf(v));
        wl[i] = v;
      }
      for (int hi = t; hi < NH; hi += 256) {
        const int hx = hi % HX, hy = (hi / HX) % HY, hz = hi / (HX * HY);
        const int sz = ND == 3 ? z0 - 1 + hz : 0, sy = y0 - 1 + hy, sx = x0 - 1 + hx;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
        if (sz >= 0 && sz < a.D0 && sy >= 0 && sy < a.D1 && sx >= 0 && sx < a.D2) {
          const int64_t off = (img + ((int64_t)sz * a.D1 + sy) * a.D2 + sx) * a.dzcs + f0;
          if constexpr (DT == 1) {
            float f[8];
            unpack8(*(const u32x4*)((const bf16_t*)a.dz + off), f);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v0[j] = f[j]; v1[j] = f[4 + j]; }
          } else {
            const float* pz = (const float*)a.dz + off;
            if (a.vec) {   // the stride is a multiple of 4 > f0 + 4 h, so each 16-byte piece lies inside the voxel
              v0 = *(const f32x4*)pz;
              if (f0 + 4 < a.F) v1 = *(const f32x4*)(pz + 4);
#pragma unroll
              for (int j = 0; j < 4; ++j) {   // lanes beyond F are padding of the caller's: never used
                if (f0 + j >= a.F) v0[j] = 0.f;
                if (f0 + 4 + j >= a.F) v1[j] = 0.f;
              }
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                if (f0 + j < a.F) v0[j] = pz[j];
                if (f0 + 4 + j < a.F) v1[j] = pz[4 + j];
              }
            }
          }
        }
        tile[0][hi] = v0;
        tile[1][hi] = v1;
      }
      __syncthreads();
#pragma unroll
      for (int kz = 0; kz < (ND == 3 ? 3 : 1); ++kz)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int tap = (kz * 3 + ky) * 3 + kx;
            const int hz = ND == 3 ? lz + 2 - kz : 0;
            const int hi = (hz * HY + (ly + 2 - ky)) * HX + (lx + 2 - kx);
            const f32x4 d0 = tile[0][hi], d1 = tile[1][hi];
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
              const f32x4 w0 = *(const f32x4*)&wl[(tap * CB + cb) * 8], w1 = *(const f32x4*)&wl[(tap * CB + cb) * 8 + 4];
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[cb] = fmaf(d0[j], w0[j], acc[cb]);
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[cb] = fmaf(d1[j], w1[j], acc[cb]);
            }
          }
    }
    if (inside) {
      float* o = a.out + (img + ((int64_t)gz * a.D1 + gy) * a.D2 + gx) * a.cin + c0;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
        if (c0 + cb < a.cin) o[cb] = acc[cb];
    }
  }
}

int launch_conv0_input_grad(int32_t ndim, const int32_t* spatial, int32_t n, int32_t cin, int32_t F, const void* dz, int32_t dz_cstride,
                            int32_t dtype, const float* w, float* dinput_out, hipStream_t s) {
  URSN_REQUIRE(spatial && dz && w && dinput_out, "conv0_input_grad: null spatial / dz / w / dinput_out");
  URSN_REQUIRE(ndim == 2 || ndim == 3, "conv0_input_grad: ndim %d not in {2, 3}", (int)ndim);
  int64_t voxels = 1;
  for (int j = 0; j < ndim; ++j) {
    URSN_REQUIRE(spatial[j] >= 1, "conv0_input_grad: spatial[%d] = %d < 1", j, (int)spatial[j]);
    voxels *= spatial[j];
    URSN_REQUIRE(voxels < ((int64_t)1 << 31), "conv0_input_grad: %lld voxels >= 2^31", (long long)voxels);
  }
  URSN_TRY(xl_check_dims("conv0_input_grad", n, voxels));
  URSN_REQUIRE(cin >= 1 && cin <= 65536, "conv0_input_grad: cin = %d outside [1, 65536]", (int)cin);
  URSN_REQUIRE(F >= 1 && F <= 65536, "conv0_input_grad: F = %d outside [1, 65536]", (int)F);
  URSN_REQUIRE(dtype == 0 || dtype == 1, "conv0_input_grad: dtype %d not in {0 fp32, 1 bf16}", (int)dtype);
  URSN_REQUIRE(dz_cstride >= F, "conv0_input_grad: dz_cstride %d < F %d", (int)dz_cstride, (int)F);
  if (dtype == 1) {
    URSN_REQUIRE(cin == 1, "conv0_input_grad: the bf16 plan has one input channel (cin = %d)", (int)cin);
    URSN_REQUIRE(F % 8 == 0 && dz_cstride % 8 == 0, "conv0_input_grad: bf16 dz needs F and dz_cstride multiples of 8 (%d, %d)", (int)F, (int)dz_cstride);
    URSN_REQUIRE(((uintptr_t)dz & 15) == 0, "conv0_input_grad: bf16 dz must be 16-byte aligned");
  } else {
    URSN_REQUIRE(((uintptr_t)dz & 3) == 0, "conv0_input_grad: fp32 dz must be 4-byte aligned");
  }
  URSN_REQUIRE((((uintptr_t)w | (uintptr_t)dinput_out) & 3) == 0, "conv0_input_grad: w / dinput_out must be 4-byte aligned");
  C0Args a;
  a.dz = dz; a.w = w; a.out = dinput_out;
  a.D0 = ndim == 3 ? spatial[0] : 1; a.D1 = spatial[ndim - 2]; a.D2 = spatial[ndim - 1];
  a.cin = cin; a.F = F; a.dzcs = dz_cstride;
  a.vec = dtype == 0 && (dz_cstride & 3) == 0 && ((uintptr_t)dz & 15) == 0;
  const int TZ = ndim == 3 ? C0Tile<3>::TZ : 1, TY = ndim == 3 ? C0Tile<3>::TY : C0Tile<2>::TY, TX = 16;
  a.nty = (a.D1 + TY - 1) / TY; a.ntx = (a.D2 + TX - 1) / TX;
  const int64_t tiles = (int64_t)((a.D0 + TZ - 1) / TZ) * a.nty * a.ntx;
  URSN_REQUIRE(tiles < ((int64_t)1 << 31), "conv0_input_grad: %lld tiles per event", (long long)tiles);
  const dim3 grid((unsigned)tiles, (unsigned)n), blk(256);
  ursn_note_kernel("conv0_input_grad");
#define C0_LAUNCH(nd, dt, cb) hipLaunchKernelGGL((conv0_input_grad_kernel<nd, dt, cb>), grid, blk, 0, s, a)
  if (ndim == 3) {
    if (dtype == 1) C0_LAUNCH(3, 1, 1);
    else if (cin == 1) C0_LAUNCH(3, 0, 1);
    else C0_LAUNCH(3, 0, 4);
  } else {
    if (dtype == 1) C0_LAUNCH(2, 1, 1);
    else if (cin == 1) C0_LAUNCH(2, 0, 1);
    else C0_LAUNCH(2, 0, 4);
  }
#undef C0_LAUNCH
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_conv0_input_grad(int32_t ndim, const int32_t* spatial, int32_t n, int32_t cin, int32_t F, const void* dz,
                                     int32_t dz_cstride, int32_t dtype, const float* w, float* dinput_out, void* stream) {
  return launch_conv0_input_grad(ndim, spatial, n, cin, F, dz, dz_cstride, dtype, w, dinput_out, (hipStream_t)stream);
}
