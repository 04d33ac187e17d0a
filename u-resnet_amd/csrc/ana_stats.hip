// Per-event, per-class analysis statistics (gfx950): ursn_class_stats forms, for every event of a batch, the confusion matrix of
// label against predicted class, the counts of labels outside [0, C) and of data > 0 voxels, and the fp64 sum / sum of squares of
// each class's softmax score over the voxels that carry the class -- what example_scripts/ana_csv.py:67-116 computes on the host
// from the dense softmax.  A stateless op-level pass like those of voxel_io.hip and weight_norm.hip: one HBM-bound streaming
// launch over conv2's stored logits plus a small reduction launch, no global atomics, no workgroup waits on another, nothing read
// that the same call did not write (the scratch buffer needs no initialisation), so the same arguments give the same bits.
#include "bf16_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// A workgroup owns a fixed span of CSTATS_SPAN consecutive voxels of one event (blockIdx.x = span, blockIdx.y = event): the span
// is a compile-time constant, so which values meet in which partial sum never depends on the launch geometry.  Thread t takes
// voxel  span start + 256 j + t  in step j = 0 .. CSTATS_ROUNDS * CSTATS_ITER - 1; the loads of CSTATS_ITER steps are in flight
// together.
#define CSTATS_ITER 8
#define CSTATS_ROUNDS 2
#define CSTATS_SPAN (256 * CSTATS_ITER * CSTATS_ROUNDS)

static inline int64_t cstats_blocks(int64_t voxels) { return cdiv64(voxels, CSTATS_SPAN); }
// Classes are padded to NC = 4 | 8 (the kernels' compile-time loop bound).  Per event and span the scratch holds 2 NC doubles
// (score sums, then sums of squares) and NC * NC + 4 uint32 counts (bin t * NC + p, then other {> 0, rest}, nonzero {data > 0,
// of those correct}); a span has 4096 voxels, so 32 bits are plenty.  Layout [event][quantity][span]: doubles first.
static inline int cstats_nc(int ncls) { return ncls <= 4 ? 4 : 8; }
static inline int cstats_nint(int nc) { return nc * nc + 4; }

struct CStatsArgs {
  ursn_vscores_desc d;   // offsets / index unused
  const float* label;
  double* pd;            // [n][2 NC][B]
  uint32_t* pc;          // [n][NC NC + 4][B]
};

// The per-voxel arithmetic RESTATES vscores_kernel (voxel_io.hip), which restates the dense heads (head_kernel in elementwise.hip,
// bhead_kernel in bf16_elementwise.hip) statement by statement: fmaf(raw, sc, sh) with sh = beta - mean * sc, strict '>' argmax,
// exp(z - m) summed in class order, e * (1 / sum).  DT: 0 fp32 logits and expf, 1 bf16 logits and __expf.  V4: <= 4 classes in
// 4-padded, 16-byte aligned fp32 logits, one 16-byte load.  NC: 4 | 8, >= ncls.
//
// Counts: every lane of a wave holds one bin of the (label, prediction) histogram.  Per step, ballots of the bits of
// bin = t * NC + p are combined per lane into the mask of the lanes whose voxel falls into THIS lane's bin; its popcount is the
// bin's share.  No per-thread counter array, no LDS atomics.  Sums: per-thread fp64 accumulators with compile-time indices
// (predicated adds over k), then lanes by shuffles and the four waves through LDS, all in a fixed order.
template <int DT, bool V4, int NC>
__global__ __launch_bounds__(256) void cstats_kernel(CStatsArgs a) {
  constexpr int NB = NC == 4 ? 4 : 6;   // bits of a bin index
  constexpr int NI = NC * NC + 4;
  __shared__ double smd[4][2 * NC];
  __shared__ uint32_t smc[4][NI];
  const ursn_vscores_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ncls = d.ncls;
  const int64_t V = d.voxels;
  const int64_t lo = (int64_t)blockIdx.x * CSTATS_SPAN;
  const int64_t base = (int64_t)blockIdx.y * V;
  const bool has_data = d.data != nullptr;
  float sc[NC], sh[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    sc[k] = 1.f;
    sh[k] = 0.f;
    if (k < ncls && d.mean) {
      sc[k] = d.rstd[k];
      sh[k] = d.beta[k] - d.mean[k] * sc[k];
    }
  }
  double as[NC], aq[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) as[k] = aq[k] = 0.0;
  uint32_t bin_cnt = 0, o_pos = 0, o_rest = 0, nz = 0, nz_ok = 0;

  for (int r = 0; r < CSTATS_ROUNDS; ++r) {
    float raw[CSTATS_ITER][NC], lab[CSTATS_ITER], dat[CSTATS_ITER];
#pragma unroll
    for (int i = 0; i < CSTATS_ITER; ++i) {
      const int64_t v = lo + (int64_t)(r * CSTATS_ITER + i) * 256 + t;
#pragma unroll
      for (int k = 0; k < NC; ++k) raw[i][k] = 0.f;
      lab[i] = 0.f;
      dat[i] = 0.f;
      if (v < V) {
        const int64_t p = base + v;
        if constexpr (DT == 1) {
          float r8[8];
          unpack8(*(const u32x4*)((const bf16_t*)d.z + p * 8), r8);
#pragma unroll
          for (int k = 0; k < NC; ++k) raw[i][k] = r8[k];
        } else if constexpr (V4) {
          const f32x4 zv = *(const f32x4*)((const float*)d.z + p * 4);
#pragma unroll
          for (int k = 0; k < NC; ++k) raw[i][k] = k < 4 ? zv[k & 3] : 0.f;
        } else {
          const float* zp = (const float*)d.z + p * d.z_cstride;
#pragma unroll
          for (int k = 0; k < NC; ++k) raw[i][k] = k < ncls ? zp[k] : 0.f;
        }
        lab[i] = a.label[p];
        if (has_data) dat[i] = d.data[p];
      }
    }
#pragma unroll
    for (int i = 0; i < CSTATS_ITER; ++i) {
      const int64_t v = lo + (int64_t)(r * CSTATS_ITER + i) * 256 + t;
      const bool inb = v < V;
      float z[NC], ex[NC];
      float m = -INFINITY;
      int arg = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k < ncls) {
          z[k] = fmaf(raw[i][k], sc[k], sh[k]);
          if (z[k] > m) { m = z[k]; arg = k; }   // strict '>' keeps the lowest index on ties
        }
      float ssum = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k < ncls) {
          if constexpr (DT == 1) ex[k] = __expf(z[k] - m);
          else ex[k] = expf(z[k] - m);
          ssum += ex[k];
        }
      const float inv = 1.0f / ssum;
      // (int)label truncates toward zero (head_kernel): the classes are the labels in (-1, ncls); NaN fails both comparisons
      const float lf = lab[i];
      const bool inr = inb && lf > -1.0f && lf < (float)ncls;
      const int tc = inr ? (int)lf : 0;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k < ncls && k == tc) s = ex[k] * inv;
      const double ds = (double)s, dq = ds * ds;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const bool hit = inr && k == tc;
        as[k] += hit ? ds : 0.0;
        aq[k] += hit ? dq : 0.0;
      }
      const int bin = tc * NC + arg;
      unsigned long long mk = __ballot(inr);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const unsigned long long bb = __ballot((bin >> b) & 1);
        mk &= ((lane >> b) & 1) ? bb : ~bb;
      }
      bin_cnt += (uint32_t)__popcll(mk);
      o_pos += (uint32_t)__popcll(__ballot(inb && !inr && lf > 0.f));
      o_rest += (uint32_t)__popcll(__ballot(inb && !inr && !(lf > 0.f)));
      const bool isnz = inb && dat[i] > 0.f;   // lib/ssnet.py:59
      nz += (uint32_t)__popcll(__ballot(isnz));
      nz_ok += (uint32_t)__popcll(__ballot(isnz && inr && arg == tc));
    }
  }

#pragma unroll
  for (int k = 0; k < NC; ++k) {
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
      as[k] += __shfl_down(as[k], dd, 64);
      aq[k] += __shfl_down(aq[k], dd, 64);
    }
    if (lane == 0) {
      smd[wave][k] = as[k];
      smd[wave][NC + k] = aq[k];
    }
  }
  if (lane < NC * NC) smc[wave][lane] = bin_cnt;
  if (lane == 0) {
    smc[wave][NC * NC + 0] = o_pos;
    smc[wave][NC * NC + 1] = o_rest;
    smc[wave][NC * NC + 2] = nz;
    smc[wave][NC * NC + 3] = nz_ok;
  }
  __syncthreads();
  const int64_t B = gridDim.x;
  if (t < 2 * NC)
    a.pd[((int64_t)blockIdx.y * (2 * NC) + t) * B + blockIdx.x] = ((smd[0][t] + smd[1][t]) + smd[2][t]) + smd[3][t];
  if (t < NI) a.pc[((int64_t)blockIdx.y * NI + t) * B + blockIdx.x] = smc[0][t] + smc[1][t] + smc[2][t] + smc[3][t];
}

// launch 2: workgroup (quantity q, event e) reduces the B per-span partials of one quantity: thread t takes partials t, t + 256,
// ... in order, then lanes by shuffles and the four waves through LDS in wave order.  Counts are integers: exact in any order.
struct CStatsFinalArgs {
  const double* pd;
  const uint32_t* pc;
  int64_t B;
  int ncls, nc;
  ursn_class_stats_out out;
};

__global__ __launch_bounds__(256) void cstats_final_kernel(CStatsFinalArgs a) {
  __shared__ double smd[4];
  __shared__ long long smi[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int q = blockIdx.x, e = blockIdx.y;
  const int nc = a.nc, C = a.ncls, ni = nc * nc + 4;
  if (q < ni) {
    const uint32_t* P = a.pc + ((int64_t)e * ni + q) * a.B;
    long long acc = 0;
    for (int64_t i = t; i < a.B; i += 256) acc += (long long)P[i];
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) acc += __shfl_down(acc, dd, 64);
    if (lane == 0) smi[wave] = acc;
    __syncthreads();
    if (t != 0) return;
    const long long tot = smi[0] + smi[1] + smi[2] + smi[3];
    if (q < nc * nc) {
      const int tl = q / nc, pr = q % nc;
      if (tl < C && pr < C) a.out.conf[((int64_t)e * C + tl) * C + pr] = tot;
    } else if (q < nc * nc + 2) {
      if (a.out.other) a.out.other[(int64_t)e * 2 + (q - nc * nc)] = tot;
    } else {
      if (a.out.nonzero) a.out.nonzero[(int64_t)e * 2 + (q - nc * nc - 2)] = tot;
    }
  } else {
    const int k2 = q - ni;   // [0, nc): score_sum, [nc, 2 nc): score_sq
    const double* P = a.pd + ((int64_t)e * (2 * nc) + k2) * a.B;
    double acc = 0.0;
    for (int64_t i = t; i < a.B; i += 256) acc += P[i];
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) acc += __shfl_down(acc, dd, 64);
    if (lane == 0) smd[wave] = acc;
    __syncthreads();
    if (t != 0) return;
    const double tot = ((smd[0] + smd[1]) + smd[2]) + smd[3];
    const int k = k2 < nc ? k2 : k2 - nc;
    double* o = k2 < nc ? a.out.score_sum : a.out.score_sq;
    if (k < C && o) o[(int64_t)e * C + k] = tot;
  }
}

static inline bool cstats_dims_ok(int32_t n, int64_t voxels, int32_t ncls) {
  return n >= 1 && n <= 65535 && voxels >= 1 && voxels < ((int64_t)1 << 31) && ncls >= 1 && ncls <= 8;
}

extern "C" size_t ursn_class_stats_scratch_bytes(int32_t n, int64_t voxels, int32_t ncls) {
  if (!cstats_dims_ok(n, voxels, ncls)) return 0;
  const int nc = cstats_nc(ncls);
  return (size_t)n * (size_t)cstats_blocks(voxels) * ((size_t)2 * nc * sizeof(double) + (size_t)cstats_nint(nc) * sizeof(uint32_t));
}

int launch_cstats(const ursn_vscores_desc* d, const float* label, const ursn_class_stats_out* out, void* scratch,
                  size_t scratch_bytes, hipStream_t s) {
  URSN_REQUIRE(d, "class_stats: null desc");
  URSN_REQUIRE(label, "class_stats: null label");
  URSN_REQUIRE(out, "class_stats: null out");
  URSN_REQUIRE(out->conf, "class_stats: null out->conf");
  URSN_REQUIRE(scratch, "class_stats: null scratch");
  URSN_REQUIRE(d->z, "class_stats: null z");
  URSN_REQUIRE(d->n >= 1 && d->n <= 65535, "class_stats: n = %d outside [1, 65535]", (int)d->n);
  URSN_REQUIRE(d->voxels >= 1, "class_stats: voxels = %lld < 1", (long long)d->voxels);
  URSN_REQUIRE(d->voxels < ((int64_t)1 << 31), "class_stats: voxels = %lld >= 2^31", (long long)d->voxels);
  URSN_REQUIRE(d->ncls >= 1 && d->ncls <= 8, "class_stats: ncls = %d not in [1, 8]", (int)d->ncls);
  URSN_REQUIRE(d->dtype == 0 || d->dtype == 1, "class_stats: dtype %d not in {0 fp32, 1 bf16}", (int)d->dtype);
  if (d->dtype == 1) {
    URSN_REQUIRE(d->z_cstride == 8, "class_stats: bf16 logits need channel stride 8 (z_cstride = %d)", (int)d->z_cstride);
    URSN_REQUIRE(((uintptr_t)d->z & 15) == 0, "class_stats: bf16 z must be 16-byte aligned");
  } else {
    URSN_REQUIRE(d->z_cstride >= d->ncls, "class_stats: z_cstride %d < ncls %d", (int)d->z_cstride, (int)d->ncls);
    URSN_REQUIRE(((uintptr_t)d->z & 3) == 0, "class_stats: fp32 z must be 4-byte aligned");
  }
  URSN_REQUIRE(!d->mean || (d->rstd && d->beta), "class_stats: mean without rstd / beta");
  URSN_REQUIRE(!out->nonzero || d->data, "class_stats: out->nonzero needs data (the data > 0 mask)");
  URSN_REQUIRE((((uintptr_t)label | (uintptr_t)d->data) & 3) == 0, "class_stats: label / data must be 4-byte aligned");
  URSN_REQUIRE((((uintptr_t)out->conf | (uintptr_t)out->other | (uintptr_t)out->nonzero | (uintptr_t)out->score_sum |
                 (uintptr_t)out->score_sq) & 7) == 0,
               "class_stats: conf / other / nonzero / score_sum / score_sq must be 8-byte aligned");
  const size_t need = ursn_class_stats_scratch_bytes(d->n, d->voxels, d->ncls);
  URSN_REQUIRE(scratch_bytes >= need, "class_stats: scratch_bytes = %zu is too small, %zu needed", scratch_bytes, need);
  URSN_REQUIRE(((uintptr_t)scratch & 7) == 0, "class_stats: scratch must be 8-byte aligned");
  const int nc = cstats_nc(d->ncls);
  const int64_t B = cstats_blocks(d->voxels);
  CStatsArgs a;
  a.d = *d;
  a.label = label;
  a.pd = (double*)scratch;
  a.pc = (uint32_t*)(a.pd + (size_t)d->n * B * 2 * nc);
  const dim3 grid((unsigned)B, (unsigned)d->n);
  ursn_note_kernel("cstats");
  if (d->dtype == 1) {
    if (nc == 4) hipLaunchKernelGGL((cstats_kernel<1, false, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((cstats_kernel<1, false, 8>), grid, dim3(256), 0, s, a);
  } else if (d->z_cstride == 4 && d->ncls <= 4 && ((uintptr_t)d->z & 15) == 0) {
    hipLaunchKernelGGL((cstats_kernel<0, true, 4>), grid, dim3(256), 0, s, a);
  } else if (nc == 4) {
    hipLaunchKernelGGL((cstats_kernel<0, false, 4>), grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((cstats_kernel<0, false, 8>), grid, dim3(256), 0, s, a);
  }
  URSN_HIP(hipGetLastError());
  CStatsFinalArgs f;
  f.pd = a.pd, f.pc = a.pc, f.B = B, f.ncls = d->ncls, f.nc = nc, f.out = *out;
  ursn_note_kernel("cstats_final");
  hipLaunchKernelGGL(cstats_final_kernel, dim3((unsigned)(cstats_nint(nc) + 2 * nc), (unsigned)d->n), dim3(256), 0, s, f);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_class_stats(const ursn_vscores_desc* d, const float* label, const ursn_class_stats_out* out, void* scratch,
                                size_t scratch_bytes, void* stream) {
  return launch_cstats(d, label, out, scratch, scratch_bytes, (hipStream_t)stream);
}
