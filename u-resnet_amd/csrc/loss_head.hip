// Device loss head (gfx950): focal exponent, label smoothing and a batch soft-Dice term beside the reference's weighted softmax
// cross-entropy, computed from conv2's stored operands straight into the plan's d(logits) tensor (ursn_loss_head; the definition
// is stated once in include/uresnet_hip.h and in losses.py).  head_kernel / bhead_kernel are the benchmark's kernels and stay
// untouched: this file RESTATES them, as ext_loss.hip does -- the partition (one thread per voxel, grid-stride over head_blocks
// workgroups of 256: every thread sees its voxels in the order the heads' threads see theirs), the logits, the strict '>' argmax,
// the fp64 block partials and their tree, the three stored layouts of dlogits_pack_kernel, and the BatchNorm-backward partials
// taken from the STORED values.  Under the neutral spec (gamma 0, smoothing 0, no Dice, no ignored label) the per-voxel statements
// are the heads' own, so the stored dlogits, the metrics and the partials carry their bits.
//   no Dice : loss_head_kernel<.., 0> (loss, accuracies, dlogits, partials in one pass over z) + loss_final_kernel
//   Dice    : loss_head_kernel<.., 1> (loss, accuracies, I_c / S_c / Y_c partials) + loss_final_kernel (metrics and the per-class
//             coefficients a_c, b_c) + loss_head_kernel<.., 2> (softmax recomputed from z, dlogits, partials)
// No atomics, no workgroup waits on another, the scratch needs no initialisation: the same arguments give the same bits.
#include <math.h>
#include <string.h>

#include "bf16_common.h"
#include "loss_head.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LossArgs {
  const void* z; int zcs;
  const float *mean, *rstd, *beta, *data, *label, *weight;
  int n; int64_t P; int ncls;
  float gamma, smoothing, dice_w;
  int gmode;      // 0: gamma == 0, 1: gamma == 1, 2: gamma == 2, 3: any other gamma > 1
  int ignore, neutral;
  void* out; int ocs, ov4;
  double* part4;        // [blocks][4]: sum w f ce, voxels with pred == label, voxels with data > 0, both
  double* dpart;        // [blocks][24]: I_c, S_c, Y_c
  double* bs;           // [blocks][3][C] or null
  const float* coef;    // [16]: a_c, b_c (gradient pass of the Dice term)
};

// the heads' tree over the 256 threads of a workgroup for four columns held in sm
__device__ __forceinline__ void lh_tree4(double (*sm)[256]) {
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if (threadIdx.x < st)
      for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + st];
    __syncthreads();
  }
}

// ZM 0: fp32 z, any stride, scalar loads.  1: fp32 z, stride 4 | 8, 16-byte aligned: 16-byte loads.  2: bf16 bit patterns, stride 8
// (and, under the neutral spec, the fast __expf / __logf of bhead_kernel).  OBF: the stored dlogits are bf16 at stride 8.  PASS: see the head of the file.
template <int ZM, bool OBF, int PASS>
__global__ __launch_bounds__(256) void loss_head_kernel(LossArgs a) {
  constexpr bool FAST = ZM == 2;
  constexpr int BC = OBF ? 8 : 4;   // channels of the BatchNorm-backward partials
  const int ncls = a.ncls;
  double loss = 0.0;
  unsigned n_ok = 0, n_nz = 0, n_ok_nz = 0;
  float sc[8], sh[8], mu[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sc[k] = 1.f;
    sh[k] = 0.f;
    mu[k] = 0.f;
    if (k < ncls && a.mean) {
      sc[k] = a.rstd[k];
      sh[k] = a.beta[k] - a.mean[k] * sc[k];
      mu[k] = a.mean[k];
    }
  }
  const float invn = 1.0f / (float)a.n;
  float bg[BC], bgx[BC];   // per-thread sums of a few hundred terms at most: fp32, as in the heads
#pragma unroll
  for (int k = 0; k < BC; ++k) bg[k] = bgx[k] = 0.f;
  float dI[8], dS[8];
  unsigned dY[8];
  float ca[8], cb[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    dI[k] = dS[k] = 0.f;
    dY[k] = 0u;
    ca[k] = cb[k] = 0.f;
    if (PASS == 2 && k < ncls) { ca[k] = a.coef[k]; cb[k] = a.coef[8 + k]; }
  }
  const bool store = PASS != 1 && a.out != nullptr;
  // bhead_kernel's fast __expf / __logf where its bits are owed (bf16 z, neutral spec); expf / logf everywhere else: the other specs
  // subtract nearly equal terms (q_k - smoothing / C), where the fast form's ~1e-6 would show in a bf16 rounding
  const bool fast = FAST && a.neutral;

  auto voxel = [&](const int64_t p, const float (&raw)[8], const float labf, const float w, const float df) {
    float z[8], e[8];
    float m = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < ncls) {
        z[k] = fmaf(raw[k], sc[k], sh[k]);
        if (z[k] > m) { m = z[k]; arg = k; }   // strict '>' keeps the lowest index on ties
      }
    float ssum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < ncls) { e[k] = fast ? __expf(z[k] - m) : expf(z[k] - m); ssum += e[k]; }
    const float inv = 1.0f / ssum;
    const int lab = (int)labf;   // truncates toward zero, as the heads do
    const bool lab_ok = lab >= 0 && lab < ncls;
    const int labc = lab_ok ? lab : 0;
    float zl = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k == labc) zl = z[k];
    if (PASS != 2) {
      const bool okp = (arg == lab), nz = a.data ? (df > 0.f) : false;
      n_ok += okp; n_nz += nz; n_ok_nz += (okp && nz);
    }
    float g[8];
    if (a.neutral) {   // the heads' statements, word for word
      const float ce = (m + (FAST ? __logf(ssum) : logf(ssum))) - zl;
      if (PASS != 2) loss += lab_ok ? (double)(w * ce) : (double)NAN;
      // d[k] = w * invn * (e[k] * inv - onehot).  The bits depend on where the compiler contracts e * inv - onehot into one fma:
      // head_kernel does in every lane, bhead_kernel in lanes 0-6 while its lane 7 is a (packed) multiply and a subtract.  Both
      // forms are written out here, so that this kernel's own vectorisation cannot choose another; tests/test_loss_head_gpu.py
      // holds both plans to the heads' bits at 8 classes.
      const float wn = w * invn;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float oh = k == labc ? 1.f : 0.f;
        const float x = (FAST && k == 7) ? ursn_mul_rn(e[k], inv) - oh : fmaf(e[k], inv, -oh);
        g[k] = k < ncls ? wn * x : 0.f;
      }
    } else {
      const bool ign = a.ignore != -1 && lab == a.ignore;
      const bool hit = lab_ok && !ign;
      // 1 - q_l from the OTHER classes' terms: exact where q_l rounds to 1 (the focal factor's hard corner)
      float eo = 0.f, el = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) { if (k == labc) el = e[k]; else eo += e[k]; }
      const float om = eo * inv, ql = el * inv;
      const float lg = logf(ssum);
      // -log q_l = log(1 + (sum of the others) / e_l): where the label leads, log(ssum) has rounded the others' share away
      const float cel = eo < 0.5f * el ? log1pf(eo / el) : lg - (zl - m);
      float ce = cel;
      const float sm_ = a.smoothing;
      if (sm_ > 0.f) {
        float sz = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < ncls) sz += z[k] - m;
        const float ceu = lg - sz / (float)ncls;   // (1/C) sum_k -log q_k
        ce = (1.f - sm_) * cel + sm_ * ceu;
      }
      float fm1 = 0.f, f = 1.f;   // (1 - q_l)^(gamma - 1), (1 - q_l)^gamma
      if (a.gmode != 0) {
        fm1 = a.gmode == 1 ? 1.f : a.gmode == 2 ? om : om > 0.f ? expf((a.gamma - 1.f) * logf(om)) : 0.f;
        f = fm1 * om;
      }
      const float h = a.gamma * fm1 * ql * ce;
      if (PASS != 2) loss += ign ? 0.0 : lab_ok ? (double)(w * (f * ce)) : (double)NAN;
      if (PASS == 1 && !ign) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < ncls) {
            const float qk = e[k] * inv;
            dS[k] += qk;
            if (hit && k == lab) { dI[k] += qk; dY[k] += 1u; }
          }
      }
      if (PASS != 1) {
        const float wn = w * invn, soc = sm_ / (float)ncls;
        float r[8];   // Dice: d L_dice / d q_k = a_k [k == l] + b_k
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = cb[k] + (hit && k == lab ? ca[k] : 0.f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          g[k] = 0.f;
          if (k < ncls && !ign) {
            const float qk = e[k] * inv;
            // dce_k = f (q_k - t_k) - gamma (1 - q_l)^(gamma - 1) q_l ([k == l] - q_k) ce, with q_l - 1 = -(1 - q_l)
            const float dce = k == labc ? f * (sm_ - soc - om) - h * om : f * (qk - soc) + h * qk;
            g[k] = wn * dce;
            if (PASS == 2) {
              // q_k (r_k - sum_j q_j r_j) as q_k sum_j q_j (r_k - r_j) (sum q = 1): no difference of two nearly equal sums where
              // q_k rounds to 1
              float dk = 0.f;
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (j < ncls && j != k) dk = fmaf(e[j] * inv, r[k] - r[j], dk);
              g[k] = fmaf(a.dice_w * qk, dk, g[k]);
            }
          }
        }
      }
    }
    if (store) {
      if constexpr (OBF) {
        const u32x4 pk = pack8(g);
        *(u32x4*)((bf16_t*)a.out + p * 8) = pk;
        if (a.bs) {
          float dr[8];
          unpack8(pk, dr);
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (k < ncls) { bg[k] += dr[k]; bgx[k] = fmaf(dr[k], (raw[k] - mu[k]) * sc[k], bgx[k]); }
        }
      } else if (a.ov4) {
        f32x4 dv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < ncls) dv[k] = g[k];
        *(f32x4*)((float*)a.out + p * 4) = dv;
        if (a.bs) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < ncls) { bg[k] += dv[k]; bgx[k] = fmaf(dv[k], (raw[k] - mu[k]) * sc[k], bgx[k]); }
        }
      } else {
        float* op = (float*)a.out + p * a.ocs;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < ncls) op[k] = g[k];
      }
    }
  };

  auto load_z = [&](const int64_t p, float (&raw)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) raw[k] = 0.f;
    if constexpr (ZM == 2) {
      unpack8(*(const u32x4*)((const bf16_t*)a.z + p * 8), raw);
    } else if constexpr (ZM == 1) {
      const f32x4* zp = (const f32x4*)((const float*)a.z + p * a.zcs);
      const f32x4 z0 = zp[0];
#pragma unroll
      for (int k = 0; k < 4; ++k) raw[k] = z0[k];
      if (ncls > 4) {
        const f32x4 z1 = zp[1];
#pragma unroll
        for (int k = 0; k < 4; ++k) raw[4 + k] = z1[k];
      }
    } else {
      const float* zp = (const float*)a.z + p * a.zcs;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < ncls) raw[k] = zp[k];
    }
  };

  // two voxels per iteration, every load of both issued before the first use (bhead_kernel's loop: p, then p + stride -- the
  // sequence of a plain grid-stride loop, so the per-thread sums add in the heads' order)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.P; p += 2 * stride) {
    const int64_t p1 = p + stride;
    const bool two = p1 < a.P;
    float r0[8], r1[8];
    load_z(p, r0);
    load_z(two ? p1 : p, r1);
    float l0 = a.label[p], l1 = two ? a.label[p1] : 0.f;
    float w0 = 1.f, w1 = 1.f, d0 = 0.f, d1 = 0.f;
    if (a.weight) { w0 = a.weight[p]; if (two) w1 = a.weight[p1]; }
    if (a.data) { d0 = a.data[p]; if (two) d1 = a.data[p1]; }
    voxel(p, r0, l0, w0, d0);
    if (two) voxel(p1, r1, l1, w1, d1);
  }

  __shared__ double sm[4][256];
  if (PASS != 2) {
    sm[0][threadIdx.x] = loss;
    sm[1][threadIdx.x] = (double)n_ok;
    sm[2][threadIdx.x] = (double)n_nz;
    sm[3][threadIdx.x] = (double)n_ok_nz;
    lh_tree4(sm);
    if (threadIdx.x < 4) a.part4[(size_t)blockIdx.x * 4 + threadIdx.x] = sm[threadIdx.x][0];
  }
  if (PASS == 1) {   // 24 columns (I, S, Y) in six rounds of four
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = 4 * r + k;
        sm[k][threadIdx.x] = col < 8 ? (double)dI[col & 7] : col < 16 ? (double)dS[col & 7] : (double)dY[col & 7];
      }
      lh_tree4(sm);
      if (threadIdx.x < 4) a.dpart[(size_t)blockIdx.x * 24 + 4 * r + threadIdx.x] = sm[threadIdx.x][0];
    }
  }
  if (PASS != 1 && a.bs) {   // uniform; dlogits_pack_kernel's rounds: 2 BC columns (sum g, sum g xhat), third row zero
    constexpr int ROUNDS = 2 * BC / 4;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = 4 * r + k;
        sm[k][threadIdx.x] = col < BC ? (double)bg[col % BC] : (double)bgx[col % BC];
      }
      lh_tree4(sm);
      if (threadIdx.x < 4) a.bs[(size_t)blockIdx.x * 3 * BC + 4 * r + threadIdx.x] = sm[threadIdx.x][0];
    }
    if (threadIdx.x < BC) a.bs[(size_t)blockIdx.x * 3 * BC + 2 * BC + threadIdx.x] = 0.0;
  }
}

// One workgroup, a fixed assignment of block partials to threads and a fixed tree (head_final_kernel's, column for column).
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ part4, const double* __restrict__ dpart, int nblocks,
                                                         int n, int64_t pix, int ncls, double dice_w, double dice_eps,
                                                         float* __restrict__ out8, float* __restrict__ coef) {
  __shared__ double sm[4][256];
  __shared__ double tot[28];
  double s[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < nblocks; b += 256)
    for (int k = 0; k < 4; ++k) s[k] += part4[(size_t)b * 4 + k];
  for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] = s[k];
  lh_tree4(sm);
  if (threadIdx.x < 4) tot[threadIdx.x] = sm[threadIdx.x][0];
  if (dpart) {
    for (int r = 0; r < 6; ++r) {
      __syncthreads();
      for (int k = 0; k < 4; ++k) s[k] = 0.0;
      for (int b = threadIdx.x; b < nblocks; b += 256)
        for (int k = 0; k < 4; ++k) s[k] += dpart[(size_t)b * 24 + 4 * r + k];
      for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] = s[k];
      lh_tree4(sm);
      if (threadIdx.x < 4) tot[4 + 4 * r + threadIdx.x] = sm[threadIdx.x][0];
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double ce = tot[0] / (double)n;
  double dice = 0.0, total = ce;
  if (dpart) {
    double dsum = 0.0;
    for (int c = 0; c < 8; ++c) {
      float ac = 0.f, bc = 0.f;
      if (c < ncls) {
        const double I = tot[4 + c], S = tot[12 + c], Y = tot[20 + c];
        const double U = S + Y + dice_eps;
        dsum += (2.0 * I + dice_eps) / U;
        ac = (float)(-2.0 / ((double)ncls * U));
        bc = (float)((2.0 * I + dice_eps) / ((double)ncls * U * U));
      }
      coef[c] = ac;
      coef[8 + c] = bc;
    }
    dice = 1.0 - dsum / (double)ncls;
    total = ce + dice_w * dice;
  }
  out8[0] = (float)total;
  out8[1] = (float)(tot[1] / ((double)n * (double)pix));
  out8[2] = tot[2] > 0 ? (float)(tot[3] / tot[2]) : NAN;
  out8[3] = (float)tot[2];
  out8[4] = (float)ce;
  out8[5] = (float)dice;
  out8[6] = 0.f;
  out8[7] = 0.f;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// scratch: [blocks][4] + [blocks][24] doubles, then the 16 coefficient floats
size_t loss_head_scratch_bytes(int n, int64_t voxels) { return (size_t)head_blocks(n, voxels) * 28 * sizeof(double) + 64; }

extern "C" size_t ursn_loss_head_scratch_bytes(int32_t n, int64_t voxels, int32_t ncls) {
  if (n < 1 || n > 65535 || voxels < 1 || voxels >= ((int64_t)1 << 31) || ncls < 1 || ncls > 8) return 0;
  return loss_head_scratch_bytes(n, voxels);
}

static bool lh_neutral(const ursn_loss_desc& sp) {
  return sp.gamma == 0.0 && sp.smoothing == 0.0 && sp.dice_weight == 0.0 && sp.ignore_label == -1;
}

int loss_spec_check(const ursn_loss_desc* spec) {
  URSN_REQUIRE(spec, "loss_head: null spec");
  const ursn_loss_desc& sp = *spec;
  URSN_REQUIRE(isfinite(sp.gamma) && (sp.gamma == 0.0 || sp.gamma >= 1.0),
               "loss_head: gamma = %g: the focal exponent must be 0 or >= 1 (the derivative of (1 - p)^gamma is unbounded at p -> 1 in between)", sp.gamma);
  URSN_REQUIRE(sp.smoothing >= 0.0 && sp.smoothing < 1.0, "loss_head: smoothing = %g outside [0, 1)", sp.smoothing);
  URSN_REQUIRE(isfinite(sp.dice_weight) && sp.dice_weight >= 0.0, "loss_head: dice_weight = %g is negative or not finite", sp.dice_weight);
  URSN_REQUIRE(isfinite(sp.dice_eps) && sp.dice_eps > 0.0, "loss_head: dice_eps = %g is not a positive finite number", sp.dice_eps);
  return 0;
}

int loss_head_prepare(LossHeadCall& c, size_t scratch_bytes) {
  const ursn_vscores_desc& d = c.d;
  URSN_REQUIRE(d.z && c.label && c.out8 && c.scratch, "loss_head: null z / label / out8 / scratch");
  URSN_REQUIRE(d.n >= 1 && d.n <= 65535, "loss_head: n = %d outside [1, 65535]", (int)d.n);
  URSN_REQUIRE(d.voxels >= 1 && d.voxels < ((int64_t)1 << 31), "loss_head: voxels = %lld outside [1, 2^31)", (long long)d.voxels);
  URSN_REQUIRE(d.ncls >= 1 && d.ncls <= 8, "loss_head: num_class %d not in [1,8]", (int)d.ncls);
  URSN_REQUIRE(d.dtype == 0 || d.dtype == 1, "loss_head: dtype %d not in {0 fp32, 1 bf16}", (int)d.dtype);
  if (d.dtype == 1) {
    URSN_REQUIRE(d.z_cstride == 8, "loss_head: bf16 z needs channel stride 8 (z_cstride = %d)", (int)d.z_cstride);
    URSN_REQUIRE(((uintptr_t)d.z & 15) == 0, "loss_head: bf16 z must be 16-byte aligned");
  } else {
    URSN_REQUIRE(d.z_cstride >= d.ncls, "loss_head: z_cstride %d < num_class %d", (int)d.z_cstride, (int)d.ncls);
    URSN_REQUIRE(((uintptr_t)d.z & 3) == 0, "loss_head: fp32 z must be 4-byte aligned");
  }
  URSN_REQUIRE(!d.mean || (d.rstd && d.beta), "loss_head: mean without rstd / beta");
  URSN_REQUIRE((((uintptr_t)c.label | (uintptr_t)c.weight | (uintptr_t)d.data | (uintptr_t)c.out8) & 3) == 0,
               "loss_head: label / weight / data / out8 must be 4-byte aligned");
  URSN_REQUIRE(((uintptr_t)c.scratch & 7) == 0, "loss_head: scratch must be 8-byte aligned");
  URSN_TRY(loss_spec_check(&c.spec));
  const ursn_loss_desc& sp = c.spec;
  if (c.out) {
    URSN_REQUIRE(c.odt == 0 || c.odt == 1, "loss_head: out_dtype %d not in {0 fp32, 1 bf16}", c.odt);
    URSN_REQUIRE(c.ocs >= d.ncls, "loss_head: out_cstride %d < num_class %d", c.ocs, (int)d.ncls);
    if (c.odt == 1) {
      URSN_REQUIRE(c.ocs == 8, "loss_head: bf16 dlog_out needs channel stride 8 (out_cstride = %d)", c.ocs);
      URSN_REQUIRE(((uintptr_t)c.out & 15) == 0, "loss_head: bf16 dlog_out must be 16-byte aligned");
    } else {
      URSN_REQUIRE(((uintptr_t)c.out & 3) == 0, "loss_head: fp32 dlog_out must be 4-byte aligned");
    }
  }
  const bool ov4 = c.out && c.odt == 0 && c.ocs == 4 && d.ncls <= 4 && ((uintptr_t)c.out & 15) == 0;
  if (c.bs) {
    URSN_REQUIRE(c.out, "loss_head: the BatchNorm-backward partials are taken from the stored dlogits (dlog_out is null)");
    URSN_REQUIRE(d.mean && d.rstd, "loss_head: the BatchNorm-backward partials need mean / rstd");
    URSN_REQUIRE(((uintptr_t)c.bs & 7) == 0, "loss_head: the partials must be 8-byte aligned");
    URSN_REQUIRE((c.odt == 1 && d.dtype == 1) || (ov4 && d.dtype == 0 && d.z_cstride == 4 && ((uintptr_t)d.z & 15) == 0),
                 "loss_head: the partials need bf16 z and bf16 dlog_out, or fp32 z and dlog_out in the 4-padded layout (stride 4, <= 4 classes, 16-byte aligned)");
    URSN_REQUIRE(c.bs_blocks == head_blocks(d.n, d.voxels), "loss_head: %d partial blocks, the head's partition has %d", c.bs_blocks,
                 head_blocks(d.n, d.voxels));
  }
  const size_t need = loss_head_scratch_bytes(d.n, d.voxels);
  URSN_REQUIRE(scratch_bytes >= need, "loss_head: scratch too small (%zu < %zu)", scratch_bytes, need);
  c.nstages = sp.dice_weight > 0.0 && c.out ? 3 : 2;
  return 0;
}

int loss_head_stage(const LossHeadCall& c, int i, hipStream_t s, const char** name, double* bytes) {
  const ursn_vscores_desc& d = c.d;
  const ursn_loss_desc& sp = c.spec;
  const bool dice = sp.dice_weight > 0.0;
  const int nb = head_blocks(d.n, d.voxels);
  double* part4 = (double*)c.scratch;
  double* dpart = part4 + (size_t)nb * 4;
  float* coef = (float*)(dpart + (size_t)nb * 24);
  const double P = (double)d.n * (double)d.voxels;
  const double zb = d.dtype == 1 ? 16.0 : ((d.z_cstride == 4 || d.z_cstride == 8) ? 4.0 * d.z_cstride : 4.0 * d.ncls);
  const double ob = !c.out ? 0.0 : c.odt == 1 ? 16.0 : (c.ocs == 4 && d.ncls <= 4) ? 16.0 : 4.0 * d.ncls;
  const double side = 4.0 * (1 + (c.weight ? 1 : 0));
  if (i == 1) {
    if (name) *name = "lossfinal";
    if (bytes) *bytes = (double)nb * 8.0 * (dice ? 28 : 4);
    ursn_note_kernel("loss_final");
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part4, dice ? (const double*)dpart : nullptr, nb,
                       (int)d.n, (int64_t)d.voxels, (int)d.ncls, sp.dice_weight, sp.dice_eps, c.out8, coef);
    URSN_HIP(hipGetLastError());
    return 0;
  }
  LossArgs a;
  memset(&a, 0, sizeof(a));
  a.z = d.z; a.zcs = d.z_cstride; a.mean = d.mean; a.rstd = d.rstd; a.beta = d.beta; a.data = d.data;
  a.label = c.label; a.weight = c.weight; a.n = d.n; a.P = (int64_t)d.n * d.voxels; a.ncls = d.ncls;
  a.gamma = (float)sp.gamma; a.smoothing = (float)sp.smoothing; a.dice_w = (float)sp.dice_weight;
  a.gmode = sp.gamma == 0.0 ? 0 : sp.gamma == 1.0 ? 1 : sp.gamma == 2.0 ? 2 : 3;
  a.ignore = sp.ignore_label; a.neutral = lh_neutral(sp) ? 1 : 0;
  a.part4 = part4; a.dpart = dpart; a.coef = coef;
  const int pass = !dice ? 0 : i == 0 ? 1 : 2;
  if (pass != 1) {
    a.out = c.out; a.ocs = c.ocs; a.bs = c.bs;
    a.ov4 = c.out && c.odt == 0 && c.ocs == 4 && d.ncls <= 4 && ((uintptr_t)c.out & 15) == 0;
  }
  const bool obf = pass != 1 && c.out && c.odt == 1;
  const int zm = d.dtype == 1 ? 2 : ((d.z_cstride == 4 || d.z_cstride == 8) && ((uintptr_t)d.z & 15) == 0) ? 1 : 0;
  if (name) *name = pass == 1 ? "losssums" : "losshead";
  if (bytes) *bytes = P * (zb + (pass == 1 ? 0.0 : ob) + side + (pass != 2 && d.data ? 4.0 : 0.0));
  ursn_note_kernel(pass == 1 ? "loss_sums" : "loss_head");
  const dim3 grid((unsigned)nb), blk(256);
#define LH_LAUNCH(ZM, OBF, PS) hipLaunchKernelGGL((loss_head_kernel<ZM, OBF, PS>), grid, blk, 0, s, a)
#define LH_Z(OBF, PS) do { if (zm == 2) LH_LAUNCH(2, OBF, PS); else if (zm == 1) LH_LAUNCH(1, OBF, PS); else LH_LAUNCH(0, OBF, PS); } while (0)
  if (pass == 1) LH_Z(false, 1);
  else if (pass == 0) { if (obf) LH_Z(true, 0); else LH_Z(false, 0); }
  else { if (obf) LH_Z(true, 2); else LH_Z(false, 2); }
#undef LH_Z
#undef LH_LAUNCH
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_loss_head(const ursn_vscores_desc* d, const float* label, const float* weight, const ursn_loss_desc* spec,
                              void* dlog_out, int32_t out_cstride, int32_t out_dtype, double* bs_partial_or_null, int32_t bs_blocks,
                              float* out8, void* scratch, size_t scratch_bytes, void* stream) {
  URSN_REQUIRE(d && spec, "loss_head: null desc / spec");
  LossHeadCall c;
  c.d = *d; c.label = label; c.weight = weight; c.spec = *spec; c.out = dlog_out; c.ocs = out_cstride; c.odt = out_dtype;
  c.bs = bs_partial_or_null; c.bs_blocks = bs_blocks; c.out8 = out8; c.scratch = scratch; c.nstages = 0;
  URSN_TRY(loss_head_prepare(c, scratch_bytes));
  for (int i = 0; i < c.nstages; ++i) URSN_TRY(loss_head_stage(c, i, (hipStream_t)stream, nullptr, nullptr));
  return 0;
}
