// spartan_amd: K variable-base multi-scalar multiplications of one size in ONE launch chain and one round trip (sp_msm_var_many over K x n
// points that arrive with K proofs, sp_msm_points_many over K scalar vectors and one resident point set): what a verifier of many proofs of
// one circuit asks for when its K verifications advance in lock step (verifier.cc, SNARK::verify_many). A single multiplication is
// latency-bound — ~335 serial point operations of which one lane's 252 Horner doublings are most, the rest of the chip idle (msm_var.hip) — so
// K independent ones add WIDTH to every kernel and no length: the kernels of msm_var.hip with a batch dimension.
//   k_msmvm_prepare  one lane per (MSM, point), K n lanes: decode (one flag word PER MSM), multiples 1..8, signed digits [K][64][n];
//   k_msmvm_windows  grid (blocks, 64 windows, K): a block sums its 256 (point, window) terms of one MSM;
//   k_msmvm_finish   K workgroups, one per MSM: cross-block sums, Horner, encode; each writes its own 36-byte slot (32 + the flag) of the host
//                    result page and counts itself in; the last one signals (sig_make(c, K)).
//   k_msmpm_digits / _windows / _finish: the same for the resident set (window w's table slice carries 16^w: a flat sum, 32-byte slots).
// The serial critical path is that of ONE multiplication (msm_var.hip); every addition is the complete one. sp_msm_var and sp_msm_points keep
// their own kernels.
#include "internal.hpp"
#include "msm_var.hpp"

namespace {
constexpr size_t MVM_MAX_K = SP_MSM_MANY_MAX_K;          // multiplications a call (spartan_hip.h): the result area holds MVM_MAX_K x 36 bytes
constexpr size_t MVM_MAX_TERMS = SP_MSM_MANY_MAX_TERMS;  // n K of a call (1 GiB of per-point tables for sp_msm_var_many)
constexpr size_t MVM_SLOT = 36;              // sp_msm_var_many: 32 bytes of encoding + the flag word
static_assert(MVM_MAX_K * MVM_SLOT <= HMAP_SIZE - HMAP_IN, "the slots of a full batch fit the result area of the host page");

__global__ void __launch_bounds__(64) k_msmvm_prepare(const uint8_t* __restrict__ enc, const Fq* __restrict__ S, unsigned n, unsigned total /* K n */,
                                                      Pt* __restrict__ table, int8_t* __restrict__ digits /*[K][64][n]*/, int* __restrict__ bad /*[K]*/) { SP_FG_PRIO();
  const unsigned g = blockIdx.x * 64 + threadIdx.x;
  if (g >= total) return;
  const unsigned k = g / n, j = g - k * n;
  uint8_t b[32];
  for (int i = 0; i < 32; i++) b[i] = enc[32 * (size_t)g + i];
  Pt p;
  if (!pt_decompress(b, &p)) {
    atomicExch(bad + k, 1);
    p = pt_identity();
  }
  Pt T[SP_VAR_TABLE];
  pt_var_table(p, T);
  for (int m = 0; m < SP_VAR_TABLE; m++) table[(size_t)g * SP_VAR_TABLE + m] = T[m];
  int8_t d[SP_VAR_WINDOWS];
  fq_signed_digits4(fq_from_mont(ld_fq(S + g)), d);
  int8_t* dk = digits + (size_t)k * SP_VAR_WINDOWS * n;
  for (int w = 0; w < SP_VAR_WINDOWS; w++) dk[(size_t)w * n + j] = d[w];
}

// grid (nblocks, 64 windows, K): partial[(k * 64 + w) * nblocks + blk] = sum over the block's 256 points of digit_w(S[k][j]) * P[k][j]
__global__ void __launch_bounds__(MV_BLOCK) k_msmvm_windows(const Pt* __restrict__ table, const int8_t* __restrict__ digits, size_t n,
                                                            Pt* __restrict__ partial) { SP_FG_PRIO();
  __shared__ Pt sm[MV_BLOCK / 64];
  const int t = threadIdx.x;
  const size_t w = blockIdx.y, k = blockIdx.z, j = (size_t)blockIdx.x * MV_BLOCK + t;
  Pt p = pt_identity();
  if (j < n) {
    const int d = digits[(k * SP_VAR_WINDOWS + w) * n + j];
    if (d != 0) {
      p = table[(k * n + j) * SP_VAR_TABLE + ((d < 0 ? -d : d) - 1)];
      if (d < 0) p = pt_neg(p);
    }
  }
  msmv_block_sum(p, sm, &partial[(k * SP_VAR_WINDOWS + w) * gridDim.x + blockIdx.x]);
}

// K workgroups: workgroup k finishes MSM k as k_msmv_finish finishes its one
__global__ void __launch_bounds__(256) k_msmvm_finish(const Pt* __restrict__ partial, size_t nblocks, const int* __restrict__ bad, uint8_t* __restrict__ out /*K x 36*/,
                                                      DoneSig sig) { SP_FG_PRIO();
  __shared__ Pt win[SP_VAR_WINDOWS];
  const int t = threadIdx.x, w = t >> 2, q = t & 3;
  const size_t k = blockIdx.x;
  const Pt* part = partial + k * SP_VAR_WINDOWS * nblocks;
  Pt acc = pt_identity();
  for (size_t b = q; b < nblocks; b += 4) acc = pt_add(acc, part[(size_t)w * nblocks + b]);
  acc = pt_add(acc, pt_shfl_down(acc, 2));
  acc = pt_add(acc, pt_shfl_down(acc, 1));
  if (q == 0) win[w] = acc;
  __syncthreads();
  if (t == 0) {
    Pt r = win[SP_VAR_WINDOWS - 1];
#pragma unroll 1
    for (int i = SP_VAR_WINDOWS - 2; i >= 0; i--) {
      r = pt_dbl(pt_dbl(pt_dbl(pt_dbl(r))));
      r = pt_add(r, win[i]);
    }
    uint8_t c[32];
    Pt10 r10 = pt10_load(r);
    fe10_pin(r10.X); fe10_pin(r10.Y); fe10_pin(r10.Z); fe10_pin(r10.T);
    pt10_compress(r10, c);
    uint8_t* o = out + k * MVM_SLOT;
    for (int i = 0; i < 32; i++) o[i] = c[i];
    *reinterpret_cast<int*>(o + 32) = bad[k];
  }
  signal_done(sig);
}

__global__ void __launch_bounds__(MV_BLOCK) k_msmpm_digits(const Fq* __restrict__ S, unsigned n, unsigned total /* K n */, int8_t* __restrict__ digits /*[K][64][n]*/) { SP_FG_PRIO();
  const unsigned g = blockIdx.x * MV_BLOCK + threadIdx.x;
  if (g >= total) return;
  const unsigned k = g / n, j = g - k * n;
  int8_t d[SP_VAR_WINDOWS];
  fq_signed_digits4(fq_from_mont(ld_fq(S + g)), d);
  int8_t* dk = digits + (size_t)k * SP_VAR_WINDOWS * n;
  for (int w = 0; w < SP_VAR_WINDOWS; w++) dk[(size_t)w * n + j] = d[w];
}

// grid (nblocks, 64 windows, K): partial[(k * 64 + w) * nblocks + blk] = sum over the block's 256 points of digit_w(S[k][j]) * 16^w P[j]
__global__ void __launch_bounds__(MV_BLOCK) k_msmpm_windows(const Pt* __restrict__ table, const int8_t* __restrict__ digits, size_t n,
                                                            Pt* __restrict__ partial) { SP_FG_PRIO();
  __shared__ Pt sm[MV_BLOCK / 64];
  const int t = threadIdx.x;
  const size_t w = blockIdx.y, k = blockIdx.z, j = (size_t)blockIdx.x * MV_BLOCK + t;
  Pt p = pt_identity();
  if (j < n) {
    const int d = digits[(k * SP_VAR_WINDOWS + w) * n + j];
    if (d != 0) {
      p = table[(w * n + j) * SP_VAR_TABLE + ((d < 0 ? -d : d) - 1)];
      if (d < 0) p = pt_neg(p);
    }
  }
  msmv_block_sum(p, sm, &partial[(k * SP_VAR_WINDOWS + w) * gridDim.x + blockIdx.x]);
}

// K workgroups: workgroup k adds the nparts partial sums of MSM k as k_msmp_finish adds its one's
__global__ void __launch_bounds__(256) k_msmpm_finish(const Pt* __restrict__ partial, size_t nparts, uint8_t* __restrict__ out /*K x 32*/, DoneSig sig) { SP_FG_PRIO();
  __shared__ Pt sm[4];
  const int t = threadIdx.x;
  const size_t k = blockIdx.x;
  const Pt* part = partial + k * nparts;
  Pt acc = pt_identity();
  for (size_t i = t; i < nparts; i += 256) acc = pt_add(acc, part[i]);
#pragma unroll 1
  for (int delta = 32; delta > 0; delta >>= 1) acc = pt_add(acc, pt_shfl_down(acc, delta));
  if ((t & 63) == 0) sm[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    Pt r = pt_add(pt_add(sm[0], sm[1]), pt_add(sm[2], sm[3]));
    uint8_t c[32];
    Pt10 r10 = pt10_load(r);
    fe10_pin(r10.X); fe10_pin(r10.Y); fe10_pin(r10.Z); fe10_pin(r10.T);
    pt10_compress(r10, c);
    uint8_t* o = out + 32 * k;
    for (int i = 0; i < 32; i++) o[i] = c[i];
  }
  signal_done(sig);
}

bool many_args_ok(size_t n, size_t K) { return n != 0 && K != 0 && n <= MV_MAX_N && K <= MVM_MAX_K && n * K <= MVM_MAX_TERMS; }

// the call's host inputs, back to back, where the kernels read them: the host-mapped page while they fit, else the device staging buffer
int32_t stage_inputs(sp_ctx* c, const void* a, size_t a_bytes, const void* b, size_t b_bytes, const uint8_t** d_a, const uint8_t** d_b) {
  const size_t total = a_bytes + b_bytes;
  if (total <= HMAP_GEN) {
    *d_a = (const uint8_t*)stage_small(c, 0, a, a_bytes);
    *d_b = b_bytes ? (const uint8_t*)stage_small(c, a_bytes, b, b_bytes) : nullptr;
    return SP_OK;
  }
  SPCHK(ensure_dstage(c, total));
  SPCHK(ensure_pinned(c, total));
  SPCHK(stage_in(c, 0, a, a_bytes));
  if (b_bytes) SPCHK(stage_in(c, a_bytes, b, b_bytes));
  *d_a = (const uint8_t*)c->dstage;
  *d_b = (const uint8_t*)c->dstage + a_bytes;
  return SP_OK;
}
}  // namespace

extern "C" int32_t sp_msm_var_many(sp_ctx* c, const uint8_t* points, const uint64_t* S, size_t n, size_t K, uint8_t* out, int32_t* status) {
  if (!c || !points || !S || !out || !status || !many_args_ok(n, K)) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const size_t nk = n * K, nblocks = (n + MV_BLOCK - 1) / MV_BLOCK;
  // device buffer: [table K n x 8 Pt][partial K x 64 x nblocks Pt][digits K x 64 n][K flags]
  const size_t off_part = nk * SP_VAR_TABLE * sizeof(Pt), off_dig = off_part + K * SP_VAR_WINDOWS * nblocks * sizeof(Pt);
  const size_t off_bad = (off_dig + (size_t)SP_VAR_WINDOWS * nk + 255) & ~(size_t)255, total = off_bad + ((4 * K + 255) & ~(size_t)255);
  const uint8_t *d_enc, *d_S;
  SPCHK(stage_inputs(c, points, 32 * nk, S, 32 * nk, &d_enc, &d_S));
  void* buf = nullptr;
  SPCHK(pool_alloc(c, total, &buf));
  uint8_t* base = (uint8_t*)buf;
  Pt* table = (Pt*)base;
  Pt* partial = (Pt*)(base + off_part);
  int8_t* digits = (int8_t*)(base + off_dig);
  int* bad = (int*)(base + off_bad);
  uint8_t* res = hres(c);
  if (hipMemsetAsync(bad, 0, 4 * K, c->stream) != hipSuccess) { pool_release(c, buf, total); return SP_EHIP; }
  DoneSig sig = sig_make(c, K);
  {
    const double ops = (double)K * ((double)(SP_VAR_TABLE - 1) * (double)n + (double)SP_VAR_WINDOWS * (double)(nblocks * MV_BLOCK) + 5.0 * (SP_VAR_WINDOWS - 1));
    ProfScope ps(c, PF_MSM_VAR, 64.0 * (double)nk + 32.0 * (double)K, nullptr, ops);
    hipLaunchKernelGGL(k_msmvm_prepare, dim3((unsigned)((nk + 63) / 64)), dim3(64), 0, c->stream, d_enc, (const Fq*)d_S, (unsigned)n, (unsigned)nk, table, digits, bad);
    hipLaunchKernelGGL(k_msmvm_windows, dim3((unsigned)nblocks, SP_VAR_WINDOWS, (unsigned)K), dim3(MV_BLOCK), 0, c->stream, (const Pt*)table, (const int8_t*)digits, n,
                       partial);
    hipLaunchKernelGGL(k_msmvm_finish, dim3((unsigned)K), dim3(256), 0, c->stream, (const Pt*)partial, nblocks, (const int*)bad, res, sig);
  }
  int32_t rc = sig_wait(c, sig);
  pool_release(c, buf, total);
  if (rc != SP_OK) return rc;
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  for (size_t k = 0; k < K; k++) {
    int flag;
    memcpy(&flag, res + k * MVM_SLOT + 32, 4);
    status[k] = flag ? SP_EPOINT : SP_OK;
    if (!flag) memcpy(out + 32 * k, res + k * MVM_SLOT, 32);
  }
  return SP_OK;
}

extern "C" int32_t sp_msm_points_many(sp_ctx* c, const sp_points* pts, const uint64_t* S, size_t n, size_t K, uint8_t* out) {
  if (!c || !pts || !S || !out || !many_args_ok(n, K) || n != pts->n || pts->dev != c->dev) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const size_t nk = n * K, nblocks = (n + MV_BLOCK - 1) / MV_BLOCK, nparts = (size_t)SP_VAR_WINDOWS * nblocks;
  // device buffer: [partial K x 64 x nblocks Pt][digits K x 64 n]
  const size_t off_dig = K * nparts * sizeof(Pt), total = off_dig + (size_t)SP_VAR_WINDOWS * nk;
  const uint8_t *d_S, *unused;
  SPCHK(stage_inputs(c, S, 32 * nk, nullptr, 0, &d_S, &unused));
  void* buf = nullptr;
  SPCHK(pool_alloc(c, total, &buf));
  Pt* partial = (Pt*)buf;
  int8_t* digits = (int8_t*)((uint8_t*)buf + off_dig);
  uint8_t* res = hres(c);
  DoneSig sig = sig_make(c, K);
  {
    const double ops = (double)K * ((double)SP_VAR_WINDOWS * (double)(nblocks * MV_BLOCK) + (double)nparts);
    ProfScope ps(c, PF_MSM_POINTS, 32.0 * (double)nk + 32.0 * (double)K, nullptr, ops);
    hipLaunchKernelGGL(k_msmpm_digits, dim3((unsigned)((nk + MV_BLOCK - 1) / MV_BLOCK)), dim3(MV_BLOCK), 0, c->stream, (const Fq*)d_S, (unsigned)n, (unsigned)nk, digits);
    hipLaunchKernelGGL(k_msmpm_windows, dim3((unsigned)nblocks, SP_VAR_WINDOWS, (unsigned)K), dim3(MV_BLOCK), 0, c->stream, (const Pt*)pts->table, (const int8_t*)digits, n,
                       partial);
    hipLaunchKernelGGL(k_msmpm_finish, dim3((unsigned)K), dim3(256), 0, c->stream, (const Pt*)partial, nparts, res, sig);
  }
  int32_t rc = sig_wait(c, sig);
  pool_release(c, buf, total);
  if (rc != SP_OK) return rc;
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  memcpy(out, res, 32 * K);
  return SP_OK;
}
