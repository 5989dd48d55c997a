// spartan_amd: variable-base multi-scalar multiplication, sum_j S[j] * P[j] over points that arrive WITH A PROOF (sp_msm_var):
// GroupElement::vartime_multiscalar_mul of PolyEvalProof::verify (src/dense_mlpoly.rs:382-384, C_LZ = <L, comm.C>). The points are not a
// sp_gens — there are no precomputed tables and nothing is known about them: they may repeat, be each other's negatives or the identity, so
// every addition is the complete one (pt_add, add-2008-hwcd-3) and every doubling pt_dbl.
//
// The launch is small (n = 32 at 2^10, 1024 at 2^20, 2048 at 2^22) and latency-bound, so the work is spread over (point, window) pairs with
// signed 4-bit windows (64 windows: one wavefront's worth for the recombination):
//   k_msmv_prepare   one lane per point: decode (a flag word reports an invalid encoding), the multiples 1..8 P (7 point operations), the
//                    scalar taken out of Montgomery form and recoded into 64 signed digits;
//   k_msmv_windows   one lane per (point, window), a block per (256 points, window): the lane's term is +-T[|d|] or the identity; 6 wavefront
//                    shuffle levels, then the block's 4 wavefront sums through LDS: one partial window sum per block;
//   k_msmv_finish    one block: the cross-block stage (4 lanes per window add the blocks' partial sums), then the Horner recombination of the
//                    64 window sums (4 doublings + 1 addition each) and the RFC 9496 encode on one lane; result and flag go to the host page.
// Point operations on the critical path: 7 + 8 (6 shuffle levels + 2 LDS) + ceil(nblocks / 4) + 2 + 63 * 5 + the encode, i.e. ~335 for
// n <= 1024 of which 252 are the doublings no schedule avoids; in all 7 n + 64 n + 315 operations. One round trip.
#include "internal.hpp"
#include "msm_var.hpp"

namespace {
__global__ void __launch_bounds__(64) k_msmv_prepare(const uint8_t* __restrict__ enc, const Fq* __restrict__ S, size_t n, Pt* __restrict__ table,
                                                     int8_t* __restrict__ digits /*[64][n]*/, int* __restrict__ bad) { SP_FG_PRIO();
  const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  uint8_t b[32];
  for (int k = 0; k < 32; k++) b[k] = enc[32 * j + k];
  Pt p;
  if (!pt_decompress(b, &p)) {
    atomicExch(bad, 1);
    p = pt_identity();
  }
  Pt T[SP_VAR_TABLE];
  pt_var_table(p, T);
  for (int m = 0; m < SP_VAR_TABLE; m++) table[j * SP_VAR_TABLE + m] = T[m];
  int8_t d[SP_VAR_WINDOWS];
  fq_signed_digits4(fq_from_mont(ld_fq(S + j)), d);
  for (int w = 0; w < SP_VAR_WINDOWS; w++) digits[(size_t)w * n + j] = d[w];
}

// grid (nblocks, 64 windows): partial[w * nblocks + blk] = sum over the block's 256 points of digit_w(S[j]) * P[j]
__global__ void __launch_bounds__(MV_BLOCK) k_msmv_windows(const Pt* __restrict__ table, const int8_t* __restrict__ digits, size_t n,
                                                           Pt* __restrict__ partial) { SP_FG_PRIO();
  __shared__ Pt sm[MV_BLOCK / 64];
  const int t = threadIdx.x;
  const size_t w = blockIdx.y, j = (size_t)blockIdx.x * MV_BLOCK + t;
  Pt p = pt_identity();
  if (j < n) {
    const int d = digits[w * n + j];
    if (d != 0) {
      p = table[j * SP_VAR_TABLE + ((d < 0 ? -d : d) - 1)];
      if (d < 0) p = pt_neg(p);
    }
  }
  msmv_block_sum(p, sm, &partial[w * gridDim.x + blockIdx.x]);
}

__global__ void __launch_bounds__(256) k_msmv_finish(const Pt* __restrict__ partial, size_t nblocks, const int* __restrict__ bad, uint8_t* __restrict__ out /*32 + 4*/,
                                                     DoneSig sig) { SP_FG_PRIO();
  __shared__ Pt win[SP_VAR_WINDOWS];
  const int t = threadIdx.x, w = t >> 2, q = t & 3;
  Pt acc = pt_identity();
  for (size_t b = q; b < nblocks; b += 4) acc = pt_add(acc, partial[(size_t)w * nblocks + b]);
  acc = pt_add(acc, pt_shfl_down(acc, 2));
  acc = pt_add(acc, pt_shfl_down(acc, 1));
  if (q == 0) win[w] = acc;
  __syncthreads();
  if (t == 0) {
    Pt r = win[SP_VAR_WINDOWS - 1];
#pragma unroll 1
    for (int k = SP_VAR_WINDOWS - 2; k >= 0; k--) {
      r = pt_dbl(pt_dbl(pt_dbl(pt_dbl(r))));
      r = pt_add(r, win[k]);
    }
    uint8_t c[32];
    Pt10 r10 = pt10_load(r);
    fe10_pin(r10.X); fe10_pin(r10.Y); fe10_pin(r10.Z); fe10_pin(r10.T);
    pt10_compress(r10, c);
    for (int k = 0; k < 32; k++) out[k] = c[k];
    *reinterpret_cast<int*>(out + 32) = *bad;
  }
  signal_done(sig);
}
// ---- resident point sets (sp_points, sp_msm_points): the same sum over points that do NOT change between calls — the two commitments of a
// ComputationCommitment, fixed for the lifetime of a circuit. The set is decoded once and keeps, per point, the multiples 1..8 of 16^w P for
// all 64 windows (64 KiB a point), so a multiplication is a flat sum of table entries: no decode, no table build, no Horner doublings.
//   k_points_build   one lane per point, at upload: decode (flag word as above), then per window the table of the running base and base <- 16 base;
//   k_msmp_digits    one lane per scalar: out of Montgomery form, 64 signed digits, the [64][n] layout of k_msmv_prepare;
//   k_msmp_windows   k_msmv_windows with the lane's term fetched from window w's slice of the resident table;
//   k_msmp_finish    one block: 256 lanes stride over all 64 x nblocks partial sums (they carry their weight 16^w already), 6 shuffle levels,
//                    the 4 wavefront sums through LDS, the encode on one lane; the result goes to the host page.
// Point operations on the critical path: 8 + ceil(64 nblocks / 256) + 8 + the encode. One round trip.
__global__ void __launch_bounds__(64) k_points_build(const uint8_t* __restrict__ enc, size_t n, Pt* __restrict__ table /*[64][n][8]*/, int* __restrict__ bad) {
  const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  uint8_t b[32];
  for (int k = 0; k < 32; k++) b[k] = enc[32 * j + k];
  Pt base;
  if (!pt_decompress(b, &base)) {
    atomicExch(bad, 1);
    base = pt_identity();
  }
#pragma unroll 1
  for (size_t w = 0; w < SP_VAR_WINDOWS; w++) {
    Pt T[SP_VAR_TABLE];
    pt_var_table(base, T);
    for (int m = 0; m < SP_VAR_TABLE; m++) table[(w * n + j) * SP_VAR_TABLE + m] = T[m];
    base = pt_dbl(T[SP_VAR_TABLE - 1]);  // 16 base = 2 (8 base)
  }
}

__global__ void __launch_bounds__(MV_BLOCK) k_msmp_digits(const Fq* __restrict__ S, size_t n, int8_t* __restrict__ digits /*[64][n]*/) { SP_FG_PRIO();
  const size_t j = (size_t)blockIdx.x * MV_BLOCK + threadIdx.x;
  if (j >= n) return;
  int8_t d[SP_VAR_WINDOWS];
  fq_signed_digits4(fq_from_mont(ld_fq(S + j)), d);
  for (int w = 0; w < SP_VAR_WINDOWS; w++) digits[(size_t)w * n + j] = d[w];
}

// grid (nblocks, 64 windows): partial[w * nblocks + blk] = sum over the block's 256 points of digit_w(S[j]) * 16^w P[j]
__global__ void __launch_bounds__(MV_BLOCK) k_msmp_windows(const Pt* __restrict__ table, const int8_t* __restrict__ digits, size_t n,
                                                           Pt* __restrict__ partial) { SP_FG_PRIO();
  __shared__ Pt sm[MV_BLOCK / 64];
  const int t = threadIdx.x;
  const size_t w = blockIdx.y, j = (size_t)blockIdx.x * MV_BLOCK + t;
  Pt p = pt_identity();
  if (j < n) {
    const int d = digits[w * n + j];
    if (d != 0) {
      p = table[(w * n + j) * SP_VAR_TABLE + ((d < 0 ? -d : d) - 1)];
      if (d < 0) p = pt_neg(p);
    }
  }
  msmv_block_sum(p, sm, &partial[w * gridDim.x + blockIdx.x]);
}

__global__ void __launch_bounds__(256) k_msmp_finish(const Pt* __restrict__ partial, size_t nparts, uint8_t* __restrict__ out /*32*/, DoneSig sig) { SP_FG_PRIO();
  __shared__ Pt sm[4];
  const int t = threadIdx.x;
  Pt acc = pt_identity();
  for (size_t i = t; i < nparts; i += 256) acc = pt_add(acc, partial[i]);
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
    for (int k = 0; k < 32; k++) out[k] = c[k];
  }
  signal_done(sig);
}
}  // namespace

extern "C" int32_t sp_msm_var(sp_ctx* c, const uint8_t* points, const uint64_t* S, size_t n, uint8_t out[32]) {
  if (!c || !points || !S || !out || n == 0 || n > MV_MAX_N) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const size_t nblocks = (n + MV_BLOCK - 1) / MV_BLOCK;
  // device buffer: [table n x 8 Pt][partial 64 x nblocks Pt][digits 64 n][flag]
  const size_t off_part = n * SP_VAR_TABLE * sizeof(Pt), off_dig = off_part + (size_t)SP_VAR_WINDOWS * nblocks * sizeof(Pt);
  const size_t off_bad = (off_dig + (size_t)SP_VAR_WINDOWS * n + 255) & ~(size_t)255, total = off_bad + 256;
  const uint8_t* d_enc;
  const Fq* d_S;
  if (64 * n <= HMAP_GEN) {  // proof-sized at 2^10..2^16: the kernel reads encodings and scalars straight from the host-mapped page
    d_enc = (const uint8_t*)stage_small(c, 0, points, 32 * n);
    d_S = (const Fq*)stage_small(c, 32 * n, S, 32 * n);
  } else {
    SPCHK(ensure_dstage(c, 64 * n));
    SPCHK(stage_in(c, 0, points, 32 * n));
    SPCHK(stage_in(c, 32 * n, S, 32 * n));
    d_enc = (const uint8_t*)c->dstage;
    d_S = (const Fq*)((const uint8_t*)c->dstage + 32 * n);
  }
  void* buf = nullptr;
  SPCHK(pool_alloc(c, total, &buf));
  uint8_t* base = (uint8_t*)buf;
  Pt* table = (Pt*)base;
  Pt* partial = (Pt*)(base + off_part);
  int8_t* digits = (int8_t*)(base + off_dig);
  int* bad = (int*)(base + off_bad);
  uint8_t* res = hres(c);
  if (hipMemsetAsync(bad, 0, 4, c->stream) != hipSuccess) { pool_release(c, buf, total); return SP_EHIP; }
  DoneSig sig = sig_make(c, 1);
  {
    const double ops = (double)(SP_VAR_TABLE - 1) * (double)n + (double)SP_VAR_WINDOWS * (double)(nblocks * MV_BLOCK) + 5.0 * (SP_VAR_WINDOWS - 1);
    ProfScope ps(c, PF_MSM_VAR, 64.0 * (double)n + 32.0, nullptr, ops);
    hipLaunchKernelGGL(k_msmv_prepare, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, d_enc, d_S, n, table, digits, bad);
    hipLaunchKernelGGL(k_msmv_windows, dim3((unsigned)nblocks, SP_VAR_WINDOWS), dim3(MV_BLOCK), 0, c->stream, (const Pt*)table, (const int8_t*)digits, n, partial);
    hipLaunchKernelGGL(k_msmv_finish, dim3(1), dim3(256), 0, c->stream, (const Pt*)partial, nblocks, (const int*)bad, res, sig);
  }
  int32_t rc = sig_wait(c, sig);
  pool_release(c, buf, total);
  if (rc != SP_OK) return rc;
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  int flag;
  memcpy(&flag, res + 32, 4);
  if (flag) return SP_EPOINT;
  memcpy(out, res, 32);
  return SP_OK;
}

extern "C" int32_t sp_points_upload(sp_ctx* c, const uint8_t* compressed, size_t n, sp_points** out) {
  if (!c || !compressed || !out || n == 0 || n > MV_MAX_N) return SP_EINVAL;
  *out = nullptr;
  HIPCHK(hipSetDevice(c->dev));
  SPCHK(ensure_dstage(c, 32 * n));
  SPCHK(stage_in(c, 0, compressed, 32 * n));
  const size_t table_bytes = n * SP_VAR_WINDOWS * SP_VAR_TABLE * sizeof(Pt);
  uint8_t* buf = nullptr;  // the table, then the flag word
  HIPCHK(hipMalloc((void**)&buf, table_bytes + 256));
  int* bad = (int*)(buf + table_bytes);
  int flag = 0;
  int32_t rc = hipMemsetAsync(bad, 0, 4, c->stream) == hipSuccess ? SP_OK : SP_EHIP;
  if (rc == SP_OK)
    hipLaunchKernelGGL(k_points_build, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, (const uint8_t*)c->dstage, n, (Pt*)buf, bad);
  if (rc == SP_OK) rc = fetch_out(c, bad, &flag, 4);
  if (rc == SP_OK && hipGetLastError() != hipSuccess) rc = SP_EHIP;
  if (rc == SP_OK && flag) rc = SP_EPOINT;
  sp_points* p = rc == SP_OK ? new (std::nothrow) sp_points{c->dev, n, (Pt*)buf} : nullptr;
  if (!p) {
    (void)hipFree(buf);
    return rc == SP_OK ? SP_ENOMEM : rc;
  }
  *out = p;
  return SP_OK;
}
extern "C" void sp_points_free(sp_points* p) {
  if (!p) return;
  (void)hipSetDevice(p->dev);
  (void)hipFree(p->table);  // waits for whatever still reads the table
  delete p;
}
extern "C" size_t sp_points_count(const sp_points* p) { return p ? p->n : 0; }

extern "C" int32_t sp_msm_points(sp_ctx* c, const sp_points* pts, const uint64_t* S, size_t n, uint8_t out[32]) {
  if (!c || !pts || !S || !out || n == 0 || n != pts->n || pts->dev != c->dev) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const size_t nblocks = (n + MV_BLOCK - 1) / MV_BLOCK, nparts = (size_t)SP_VAR_WINDOWS * nblocks;
  // device buffer: [partial 64 x nblocks Pt][digits 64 n]
  const size_t off_dig = nparts * sizeof(Pt), total = off_dig + (size_t)SP_VAR_WINDOWS * n;
  const Fq* d_S;
  if (32 * n <= HMAP_GEN) {
    d_S = (const Fq*)stage_small(c, 0, S, 32 * n);
  } else {
    SPCHK(ensure_dstage(c, 32 * n));
    SPCHK(stage_in(c, 0, S, 32 * n));
    d_S = (const Fq*)c->dstage;
  }
  void* buf = nullptr;
  SPCHK(pool_alloc(c, total, &buf));
  Pt* partial = (Pt*)buf;
  int8_t* digits = (int8_t*)((uint8_t*)buf + off_dig);
  uint8_t* res = hres(c);
  DoneSig sig = sig_make(c, 1);
  {
    const double ops = (double)SP_VAR_WINDOWS * (double)(nblocks * MV_BLOCK) + (double)nparts;
    ProfScope ps(c, PF_MSM_POINTS, 32.0 * (double)n + 32.0, nullptr, ops);
    hipLaunchKernelGGL(k_msmp_digits, dim3((unsigned)nblocks), dim3(MV_BLOCK), 0, c->stream, d_S, n, digits);
    hipLaunchKernelGGL(k_msmp_windows, dim3((unsigned)nblocks, SP_VAR_WINDOWS), dim3(MV_BLOCK), 0, c->stream, (const Pt*)pts->table, (const int8_t*)digits, n,
                       partial);
    hipLaunchKernelGGL(k_msmp_finish, dim3(1), dim3(256), 0, c->stream, (const Pt*)partial, nparts, res, sig);
  }
  int32_t rc = sig_wait(c, sig);
  pool_release(c, buf, total);
  if (rc != SP_OK) return rc;
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  memcpy(out, res, 32);
  return SP_OK;
}
