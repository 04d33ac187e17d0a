// Guarded optimiser step (gfx950): a deterministic segmented reduction over the flat gradient buffer, one segment per trainable
// tensor (sum g^2, sum p^2, max |g|, non-finite count), and an Adam launch that takes its decision (clip coefficient, skip) from
// the result on the device.  Op-level and stateless like weight_norm.hip: the state buffer is the caller's, no atomics, no workgroup
// waits on another, nothing is read that the same call or ursn_opt_state_init did not write, so the same arguments give the same
// bits.  Definitions: include/uresnet_hip.h, "guarded optimiser step".
#include "ursn_common.h"

#include <algorithm>
#include <math.h>
#include <string.h>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define OPT_CHUNK URSN_OPT_CHUNK          // 256 threads x 4 float4: a thread owns float4 t + 256 i of its chunk
#define OPT_ITER (OPT_CHUNK / (256 * 4))
#define OPT_MAGIC 0x4452474f5352554cLL
#define OPT_GRID 1024                     // op-level entries do not know the chunk count: the kernels stride over the table
#define OPT_MAX_SEG 65536
#define OPT_FINAL_THREADS 1024
static_assert(OPT_CHUNK == 256 * 4 * OPT_ITER, "a chunk is a whole number of float4 rounds of 256 threads");

namespace {

struct OptHeader { int64_t magic, n_seg, n_chunks, reserved_[5]; };                 // 64 bytes at offset 0
struct OptSeg { int64_t off, nelem; int32_t decay, first_chunk, n_chunks, pad_; };  // 32 bytes
struct OptChunk { int64_t off; int32_t len, seg; };                                 // 16 bytes
struct OptPartial { double gsq, psq; float gmax; uint32_t nonfinite; uint64_t pad_; };   // 32 bytes; pad_ is never written nor read
static_assert(sizeof(OptHeader) == 64 && sizeof(OptSeg) == 32 && sizeof(OptChunk) == 16 && sizeof(OptPartial) == 32, "state layout");
static_assert(sizeof(ursn_opt_status) == 48 && sizeof(ursn_opt_tensor) == 32, "state layout");

// [header 64 | status 64 | results 32 n_seg | partials 32 n_chunks | segment table 32 n_seg | chunk table 16 n_chunks]
struct OptLayout { int64_t status, results, partials, segs, chunks, bytes; };
__host__ __device__ inline OptLayout opt_layout(int64_t n_seg, int64_t n_chunks) {
  OptLayout L;
  L.status = 64;
  L.results = 128;
  L.partials = L.results + 32 * n_seg;
  L.segs = L.partials + 32 * n_chunks;
  L.chunks = L.segs + 32 * n_seg;
  L.bytes = L.chunks + 16 * n_chunks;
  return L;
}

// chunks of a tensor list, or -1 when it is out of domain
int64_t opt_count_chunks(const int64_t* nelem, int32_t n_seg) {
  if (!nelem || n_seg < 1 || n_seg > OPT_MAX_SEG) return -1;
  int64_t nc = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (nelem[i] < 1 || nelem[i] > ((int64_t)1 << 40)) return -1;
    nc += cdiv64(nelem[i], OPT_CHUNK);
  }
  return nc < ((int64_t)1 << 31) ? nc : -1;
}

// ---- launch 1: per-chunk partials ------------------------------------------------------------------------------------------
// A non-finite element contributes 0 to the sum and the maximum and is only counted.
__device__ __forceinline__ void opt_elem(float x, double& sq, float& mx, uint32_t& nf) {
  const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const float xf = fin ? x : 0.f;
  const double d = (double)xf;
  sq += d * d;   // the square of a widened fp32 is exact in fp64
  mx = fmaxf(mx, fabsf(xf));
  nf += fin ? 0u : 1u;
}

// One thread's share of a chunk of `len` <= OPT_CHUNK floats at x: h < 4 scalar elements up to the first 16-byte boundary taken
// from the ADDRESS, Q aligned float4s (thread t owns float4 t + 256 i), < 4 scalar elements of tail; in that order.
__device__ __forceinline__ void opt_chunk_thread(const float* x, int len, double& sq, float& mx, uint32_t& nf) {
  const int t = threadIdx.x;
  int h = (int)(((16 - ((uintptr_t)x & 15)) & 15) >> 2);
  if (h > len) h = len;
  const int Q = (len - h) >> 2, tail = len - h - 4 * Q;
  const f32x4* A = (const f32x4*)(x + h);
  f32x4 r[OPT_ITER];
#pragma unroll
  for (int i = 0; i < OPT_ITER; ++i)
    if (t + 256 * i < Q) r[i] = A[t + 256 * i];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  mx = 0.f;
  nf = 0u;
#pragma unroll
  for (int i = 0; i < OPT_ITER; ++i)
    if (t + 256 * i < Q) {
      opt_elem(r[i][0], a0, mx, nf);
      opt_elem(r[i][1], a1, mx, nf);
      opt_elem(r[i][2], a2, mx, nf);
      opt_elem(r[i][3], a3, mx, nf);
    }
  sq = (a0 + a1) + (a2 + a3);
  if (t < h) opt_elem(x[t], sq, mx, nf);
  if (t < tail) opt_elem(x[h + 4 * Q + t], sq, mx, nf);
}

// lanes by shuffles in a fixed order, then the four waves through LDS in wave order; the result is valid in thread 0
__device__ __forceinline__ double opt_block_sum(double acc, double* sm) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__global__ __launch_bounds__(256) void gstat_chunk_kernel(char* __restrict__ state, const float* __restrict__ g,
                                                          const float* __restrict__ p) {
  __shared__ double sm_g[4], sm_p[4];
  __shared__ float sm_mx[4];
  __shared__ uint32_t sm_nf[4];
  const OptHeader* H = (const OptHeader*)state;
  if (H->magic != OPT_MAGIC) return;   // not a state ursn_opt_state_init built: touch nothing
  const int64_t n_chunks = H->n_chunks;
  const OptLayout L = opt_layout(H->n_seg, n_chunks);
  const OptChunk* CT = (const OptChunk*)(state + L.chunks);
  OptPartial* PT = (OptPartial*)(state + L.partials);
  const int t = threadIdx.x;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {   // the trip count is uniform over the workgroup
    const OptChunk ch = CT[c];
    double gs, ps = 0.0;
    float mx, pmx;
    uint32_t nf, pnf;
    opt_chunk_thread(g + ch.off, ch.len, gs, mx, nf);
    if (p) opt_chunk_thread(p + ch.off, ch.len, ps, pmx, pnf);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      mx = fmaxf(mx, __shfl_down(mx, d, 64));
      nf += __shfl_down(nf, d, 64);
    }
    if ((t & 63) == 0) { sm_mx[t >> 6] = mx; sm_nf[t >> 6] = nf; }
    gs = opt_block_sum(gs, sm_g);
    ps = opt_block_sum(ps, sm_p);
    if (t == 0) {
      PT[c].gsq = gs;
      PT[c].psq = ps;
      PT[c].gmax = fmaxf(fmaxf(sm_mx[0], sm_mx[1]), fmaxf(sm_mx[2], sm_mx[3]));
      PT[c].nonfinite = (sm_nf[0] + sm_nf[1]) + (sm_nf[2] + sm_nf[3]);
    }
    __syncthreads();   // the LDS slots are free for the next chunk
  }
}

// ---- launch 2: per-tensor results and the status record (ONE workgroup) ---------------------------------------------------------
__device__ __forceinline__ double opt_readlane(double v, int lane) {   // `lane` is uniform over the wave
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// A wave owns a tensor: 64 chunk partials per round are loaded one per lane, parked in the wave's own LDS slot and added strictly
// in chunk order by every lane alike (uniform LDS reads, so all lanes form the same sum and the reads run ahead of the dependent
// fp64 adds); the maximum and the count do not depend on the order.  Tensors are dealt to the waves even indices first: in the net's
// table the even tensors are the weights and the odd ones the small beta vectors, so neighbouring waves share the long tensors.
// Then wave 0 adds the tensors in index order through readlane.
__global__ __launch_bounds__(OPT_FINAL_THREADS) void gstat_final_kernel(char* __restrict__ state, int with_p) {
  __shared__ double sm_part[OPT_FINAL_THREADS / 64][64][2];
  const OptHeader* H = (const OptHeader*)state;
  if (H->magic != OPT_MAGIC) return;
  const int n_seg = (int)H->n_seg;
  const OptLayout L = opt_layout(n_seg, H->n_chunks);
  const OptSeg* ST = (const OptSeg*)(state + L.segs);
  const OptPartial* PT = (const OptPartial*)(state + L.partials);
  ursn_opt_tensor* R = (ursn_opt_tensor*)(state + L.results);
  ursn_opt_status* S = (ursn_opt_status*)(state + L.status);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int half = (n_seg + 1) >> 1;
  for (int k = wave; k < n_seg; k += nwaves) {
    const int s = k < half ? 2 * k : 2 * (k - half) + 1;
    const int first = ST[s].first_chunk, nc = ST[s].n_chunks;
    double G = 0.0, P = 0.0;
    float mx = 0.f;
    unsigned long long nf = 0;
    for (int base = 0; base < nc; base += 64) {
      const int cnt = nc - base < 64 ? nc - base : 64;
      if (lane < cnt) {
        const OptPartial pt = PT[first + base + lane];
        sm_part[wave][lane][0] = pt.gsq;
        sm_part[wave][lane][1] = pt.psq;
        mx = fmaxf(mx, pt.gmax);
        nf += pt.nonfinite;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 8
      for (int j = 0; j < cnt; ++j) {
        G += sm_part[wave][j][0];
        P += sm_part[wave][j][1];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the slot is read before the next round overwrites it
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, d, 64));
      nf += __shfl_xor(nf, d, 64);
    }
    if (lane == 0) {
      R[s].g_sumsq = G;
      R[s].p_sumsq = with_p ? P : 0.0;
      R[s].g_maxabs = mx;
      R[s].reserved_ = 0;
      R[s].nonfinite = (int64_t)nf;
    }
  }
  __threadfence_block();
  __syncthreads();
  if (wave != 0) return;
  double T = 0.0;
  unsigned long long nf = 0;
  for (int base = 0; base < n_seg; base += 64) {
    const int cnt = n_seg - base < 64 ? n_seg - base : 64;
    double gq = 0.0;
    if (lane < cnt) {
      gq = R[base + lane].g_sumsq;
      nf += (unsigned long long)R[base + lane].nonfinite;
    }
    for (int j = 0; j < cnt; ++j) T += opt_readlane(gq, j);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) nf += __shfl_xor(nf, d, 64);
  if (lane == 0) {
    S->sumsq = T;
    S->norm = sqrt(T);
    S->nonfinite = (int64_t)nf;
    S->coef = 1.0f;
    S->skip = 0;   // calls and skipped_total stay: ursn_opt_state_init zeroed them, opt_decide_kernel counts
  }
}

// ---- launch 3: the decision (one thread) ----------------------------------------------------------------------------------------
__global__ void opt_decide_kernel(char* __restrict__ state, float clip_norm, int skip_nonfinite) {
  const OptHeader* H = (const OptHeader*)state;
  if (H->magic != OPT_MAGIC || threadIdx.x != 0 || blockIdx.x != 0) return;
  ursn_opt_status* S = (ursn_opt_status*)(state + 64);
  const double norm = S->norm;
  const int skip = (skip_nonfinite && S->nonfinite > 0) ? 1 : 0;
  S->coef = (clip_norm > 0.f && norm > (double)clip_norm) ? (float)((double)clip_norm / norm) : 1.0f;
  S->skip = skip;
  S->calls += 1;
  S->skipped_total += skip;
}

// ---- launch 4: Adam over the chunk table ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void opt_adam_kernel(const char* __restrict__ state, float* __restrict__ p,
                                                       const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                       int64_t n, float lr_t, float decay, float b1, float b2, float eps) {
  const OptHeader* H = (const OptHeader*)state;
  if (H->magic != OPT_MAGIC) return;
  const ursn_opt_status* S = (const ursn_opt_status*)(state + 64);
  if (S->skip) return;   // nothing of p, m, v is written
  const float coef = S->coef;
  const int64_t n_chunks = H->n_chunks;
  const OptLayout L = opt_layout(H->n_seg, n_chunks);
  const OptChunk* CT = (const OptChunk*)(state + L.chunks);
  const OptSeg* ST = (const OptSeg*)(state + L.segs);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const OptChunk ch = CT[c];
    if (ch.off < 0 || ch.off + ch.len > n) continue;   // a table that does not fit the buffers: touch nothing of that chunk
    const bool dec = ST[ch.seg].decay != 0;
    for (int i = threadIdx.x; i < ch.len; i += 256) {
      const int64_t at = ch.off + i;
      const float gi = ursn_mul_rn(g[at], coef);
      float pi = p[at], mi = m[at], vi = v[at];
      if (dec) pi = ursn_mul_rn(pi, decay);
      ursn_adam_element(pi, gi, mi, vi, lr_t, b1, b2, eps);
      p[at] = pi;
      m[at] = mi;
      v[at] = vi;
    }
  }
}

unsigned opt_grid(int64_t nchunks_hint) {
  if (nchunks_hint <= 0) return OPT_GRID;
  return (unsigned)(nchunks_hint < 65536 ? nchunks_hint : 65536);
}

int opt_check_state(const void* state, const char* what) {
  URSN_REQUIRE(state, "%s: null state", what);
  URSN_REQUIRE(((uintptr_t)state & 15) == 0, "%s: the state must be 16-byte aligned", what);
  return 0;
}

int opt_check_desc(const ursn_opt_desc* d, const char* what) {
  URSN_REQUIRE(d, "%s: null desc", what);
  URSN_REQUIRE(d->lr > 0.f && d->lr < INFINITY, "%s: lr = %g is not a positive finite number", what, (double)d->lr);
  URSN_REQUIRE(d->clip_norm == d->clip_norm, "%s: clip_norm is NaN", what);
  const double shrink = (double)d->lr * (double)d->weight_decay;
  URSN_REQUIRE(shrink >= 0.0 && shrink <= 1.0, "%s: lr * weight_decay = %g outside [0, 1]", what, shrink);
  return 0;
}

}  // namespace

int opt_launch_stats(void* state, const float* g, const float* p, int64_t nchunks_hint, hipStream_t s) {
  ursn_note_kernel("gstat_chunk");
  hipLaunchKernelGGL(gstat_chunk_kernel, dim3(opt_grid(nchunks_hint)), dim3(256), 0, s, (char*)state, g, p);
  URSN_HIP(hipGetLastError());
  ursn_note_kernel("gstat_final");
  hipLaunchKernelGGL(gstat_final_kernel, dim3(1), dim3(OPT_FINAL_THREADS), 0, s, (char*)state, p ? 1 : 0);
  URSN_HIP(hipGetLastError());
  return 0;
}

int opt_launch_adam(void* state, float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float decay,
                    int64_t nchunks_hint, hipStream_t s) {
  ursn_note_kernel("opt_adam");
  hipLaunchKernelGGL(opt_adam_kernel, dim3(opt_grid(nchunks_hint)), dim3(256), 0, s, (const char*)state, p, g, m, v, n, lr_t, decay,
                     0.9f, 0.999f, 1e-8f);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t ursn_opt_state_size(const int64_t* nelem_host, int32_t n_seg) {
  const int64_t nc = opt_count_chunks(nelem_host, n_seg);
  return nc < 0 ? 0 : (size_t)opt_layout(n_seg, nc).bytes;
}

extern "C" int ursn_opt_state_layout(const int64_t* nelem_host, int32_t n_seg, int64_t* out6) {
  URSN_REQUIRE(nelem_host && out6, "opt_state_layout: null argument");
  const int64_t nc = opt_count_chunks(nelem_host, n_seg);
  URSN_REQUIRE(nc >= 0, "opt_state_layout: n_seg = %d outside [1, %d], an element count outside [1, 2^40] or 2^31 chunks or more",
               (int)n_seg, OPT_MAX_SEG);
  const OptLayout L = opt_layout(n_seg, nc);
  out6[0] = L.bytes; out6[1] = L.status; out6[2] = L.results; out6[3] = L.partials; out6[4] = nc; out6[5] = OPT_CHUNK;
  return 0;
}

extern "C" int ursn_opt_state_init(void* state, size_t bytes, const int64_t* offsets_host, const int64_t* nelem_host,
                                   const int32_t* decay_host, int32_t n_seg) {
  URSN_TRY(opt_check_state(state, "opt_state_init"));
  URSN_REQUIRE(offsets_host && nelem_host && decay_host, "opt_state_init: null offsets / nelem / decay");
  const int64_t nc = opt_count_chunks(nelem_host, n_seg);
  URSN_REQUIRE(nc >= 0, "opt_state_init: n_seg = %d outside [1, %d], an element count outside [1, 2^40] or 2^31 chunks or more",
               (int)n_seg, OPT_MAX_SEG);
  const OptLayout L = opt_layout(n_seg, nc);
  URSN_REQUIRE(bytes >= (size_t)L.bytes, "opt_state_init: state of %zu bytes is too small, %lld needed", bytes, (long long)L.bytes);
  std::vector<int> order(n_seg);
  for (int i = 0; i < n_seg; ++i) {
    URSN_REQUIRE(offsets_host[i] >= 0 && offsets_host[i] <= ((int64_t)1 << 40), "opt_state_init: offset %lld of tensor %d out of range",
                 (long long)offsets_host[i], i);
    order[i] = i;
  }
  std::sort(order.begin(), order.end(), [&](int a, int b) { return offsets_host[a] < offsets_host[b]; });
  for (int i = 0; i + 1 < n_seg; ++i)
    URSN_REQUIRE(offsets_host[order[i]] + nelem_host[order[i]] <= offsets_host[order[i + 1]],
                 "opt_state_init: tensors %d and %d overlap", order[i], order[i + 1]);
  std::vector<OptSeg> segs(n_seg);
  std::vector<OptChunk> chunks((size_t)nc);
  int64_t c = 0;
  for (int i = 0; i < n_seg; ++i) {
    OptSeg& sg = segs[i];
    sg.off = offsets_host[i]; sg.nelem = nelem_host[i]; sg.decay = decay_host[i] != 0; sg.first_chunk = (int32_t)c;
    sg.n_chunks = (int32_t)cdiv64(nelem_host[i], OPT_CHUNK); sg.pad_ = 0;
    for (int64_t lo = 0; lo < nelem_host[i]; lo += OPT_CHUNK, ++c) {
      const int64_t left = nelem_host[i] - lo;
      chunks[(size_t)c] = {offsets_host[i] + lo, (int32_t)(left < OPT_CHUNK ? left : OPT_CHUNK), i};
    }
  }
  OptHeader H;
  memset(&H, 0, sizeof(H));
  H.magic = OPT_MAGIC; H.n_seg = n_seg; H.n_chunks = nc;
  char* base = (char*)state;
  URSN_HIP(hipMemset(base + L.status, 0, 64));
  URSN_HIP(hipMemcpy(base + L.segs, segs.data(), segs.size() * sizeof(OptSeg), hipMemcpyHostToDevice));
  URSN_HIP(hipMemcpy(base + L.chunks, chunks.data(), chunks.size() * sizeof(OptChunk), hipMemcpyHostToDevice));
  URSN_HIP(hipMemcpy(base, &H, sizeof(H), hipMemcpyHostToDevice));
  URSN_HIP(hipDeviceSynchronize());
  return 0;
}

extern "C" int ursn_opt_stats(void* state, const float* g, const float* p_or_null, void* stream) {
  URSN_TRY(opt_check_state(state, "opt_stats"));
  URSN_REQUIRE(g, "opt_stats: null gradient buffer");
  URSN_REQUIRE((((uintptr_t)g | (uintptr_t)p_or_null) & 3) == 0, "opt_stats: g / p must be 4-byte aligned");
  return opt_launch_stats(state, g, p_or_null, 0, (hipStream_t)stream);
}

extern "C" int ursn_opt_decide(void* state, const ursn_opt_desc* desc, void* stream) {
  URSN_TRY(opt_check_state(state, "opt_decide"));
  URSN_TRY(opt_check_desc(desc, "opt_decide"));
  ursn_note_kernel("opt_decide");
  hipLaunchKernelGGL(opt_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (char*)state, desc->clip_norm,
                     desc->skip_nonfinite != 0);
  URSN_HIP(hipGetLastError());
  return 0;
}

extern "C" int ursn_opt_adam(void* state, float* p, const float* g, float* m, float* v, int64_t n, const ursn_opt_desc* desc,
                             int64_t t, void* stream) {
  URSN_TRY(opt_check_state(state, "opt_adam"));
  URSN_TRY(opt_check_desc(desc, "opt_adam"));
  URSN_REQUIRE(p && g && m && v, "opt_adam: null p / g / m / v");
  URSN_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 3) == 0, "opt_adam: p / g / m / v must be 4-byte aligned");
  URSN_REQUIRE(n >= 1 && t >= 1, "opt_adam: n = %lld, t = %lld, both must be >= 1", (long long)n, (long long)t);
  const float b1 = 0.9f, b2 = 0.999f;   // the betas as ursn_adam's callers pass them: fp32, widened (the net level forms lr_t as ursn_apply_adam does)
  const double lr_t = (double)desc->lr * sqrt(1.0 - pow((double)b2, (double)t)) / (1.0 - pow((double)b1, (double)t));
  const float decay = (float)(1.0 - (double)desc->lr * (double)desc->weight_decay);
  return opt_launch_adam(state, p, g, m, v, n, (float)lr_t, decay, 0, (hipStream_t)stream);
}

extern "C" int ursn_opt_state_read(const void* state, int32_t n_seg, ursn_opt_status* status_out, ursn_opt_tensor* tensors_out,
                                   void* stream) {
  URSN_TRY(opt_check_state(state, "opt_state_read"));
  URSN_REQUIRE(status_out, "opt_state_read: null status_out");
  hipStream_t s = (hipStream_t)stream;
  char head[128];
  URSN_HIP(hipMemcpyAsync(head, state, sizeof(head), hipMemcpyDeviceToHost, s));
  URSN_HIP(hipStreamSynchronize(s));
  const OptHeader* H = (const OptHeader*)head;
  URSN_REQUIRE(H->magic == OPT_MAGIC, "opt_state_read: the state was not built by ursn_opt_state_init");
  URSN_REQUIRE(H->n_seg == n_seg, "opt_state_read: n_seg = %d, the state holds %lld tensors", (int)n_seg, (long long)H->n_seg);
  memcpy(status_out, head + 64, sizeof(*status_out));
  if (tensors_out) {
    URSN_HIP(hipMemcpyAsync(tensors_out, (const char*)state + 128, (size_t)n_seg * sizeof(ursn_opt_tensor), hipMemcpyDeviceToHost, s));
    URSN_HIP(hipStreamSynchronize(s));
  }
  return 0;
}
