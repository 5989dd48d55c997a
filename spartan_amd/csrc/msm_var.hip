// spartan_amd: variable-base multi-scalar multiplication, sum_j S[j] * P[j] over points that arrive WITH A PROOF (sp_msm_var, sp_msm_var_many):
// GroupElement::vartime_multiscalar_mul of PolyEvalProof::verify (src/dense_mlpoly.rs:382-384, C_LZ = <L, comm.C>). The points are not a
// sp_gens — there are no precomputed tables and nothing is known about them: they may repeat, be each other's negatives or the identity, so
// every addition is the complete one (pt_add, add-2008-hwcd-3) and every doubling pt_dbl.
//
// A multiplication is small (n = 32 at 2^10, 1024 at 2^20, 2048 at 2^22) and latency-bound, so the work is spread over (point, window) pairs
// with signed 4-bit windows (64 windows: one wavefront's worth for the recombination). Every kernel carries a batch dimension: a call runs K
// multiplications of one size in ONE launch chain and one round trip, which is what a verifier of many proofs of one circuit asks for when its
// K verifications advance in lock step (verifier.cc, SNARK::verify_many). K independent multiplications add WIDTH to every kernel and no
// length; sp_msm_var is the call with K = 1.
//   k_msmv_prepare   one lane per (MSM, point), K n lanes: decode (one flag word PER MSM reports an invalid encoding), the multiples 1..8 P
//                    (7 point operations), the scalar taken out of Montgomery form and recoded into 64 signed digits, [K][64][n];
//   k_msmv_windows   one lane per (point, window), grid (blocks, 64 windows, K), a block per (256 points, window) of one MSM: the lane's term
//                    is +-T[|d|] or the identity; 6 wavefront shuffle levels, then the block's 4 wavefront sums through LDS: one partial window
//                    sum per block;
//   k_msmv_finish    K workgroups, one per MSM: the cross-block stage (4 lanes per window add the blocks' partial sums), then the Horner
//                    recombination of the 64 window sums (4 doublings + 1 addition each) and the RFC 9496 encode on one lane; each writes its
//                    own 36-byte slot (32 + the flag) of the host result page and counts itself in; the last one signals (sig_make(c, K)).
// Point operations on the critical path, that of ONE multiplication whatever K: 7 + 8 (6 shuffle levels + 2 LDS) + ceil(nblocks / 4) + 2 +
// 63 * 5 + the encode, i.e. ~335 for n <= 1024 of which 252 are one lane's doublings no schedule avoids, the rest of the chip idle; in all
// K (7 n + 64 n + 315) operations.
#include "internal.hpp"

constexpr size_t MV_MAX_N = 65536;
constexpr int MV_BLOCK = 256;

namespace {
constexpr size_t MVM_MAX_K = SP_MSM_MANY_MAX_K;          // multiplications a call (spartan_hip.h): the result area holds MVM_MAX_K x 36 bytes
constexpr size_t MVM_MAX_TERMS = SP_MSM_MANY_MAX_TERMS;  // n K of a call (1 GiB of per-point tables for sp_msm_var_many)
constexpr size_t MVM_SLOT = 36;                          // k_msmv_finish: 32 bytes of encoding + the flag word
static_assert(MVM_MAX_K * MVM_SLOT <= HMAP_SIZE - HMAP_IN, "the slots of a full batch fit the result area of the host page");

__device__ __forceinline__ Pt pt_shfl_down(const Pt& p, int delta) {
  Pt r;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    r.X.v[i] = __shfl_down((unsigned long long)p.X.v[i], delta, 64);
    r.Y.v[i] = __shfl_down((unsigned long long)p.Y.v[i], delta, 64);
    r.Z.v[i] = __shfl_down((unsigned long long)p.Z.v[i], delta, 64);
    r.T.v[i] = __shfl_down((unsigned long long)p.T.v[i], delta, 64);
  }
  return r;
}

// The sum of one term per lane over a block of MV_BLOCK lanes, shared by the window kernels of sp_msm_var and sp_msm_points: 6 wavefront
// shuffle levels, then the 4 wavefront sums through LDS; lane 0 writes the block's sum. EVERY lane of the block must call it (no early exit
// before it): lane 0 of each wavefront ends with the sum of its 64 terms.
__device__ __forceinline__ void msmv_block_sum(Pt p, Pt* sm /*[MV_BLOCK / 64], shared*/, Pt* __restrict__ out) {
  const int t = threadIdx.x;
#pragma unroll 1
  for (int delta = 32; delta > 0; delta >>= 1) p = pt_add(p, pt_shfl_down(p, delta));
  if ((t & 63) == 0) sm[t >> 6] = p;
  __syncthreads();
  if (t == 0) *out = pt_add(pt_add(sm[0], sm[1]), pt_add(sm[2], sm[3]));
}

__global__ void __launch_bounds__(64) k_msmv_prepare(const uint8_t* __restrict__ enc, const Fq* __restrict__ S, unsigned n, unsigned total /* K n */,
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
__global__ void __launch_bounds__(MV_BLOCK) k_msmv_windows(const Pt* __restrict__ table, const int8_t* __restrict__ digits, size_t n,
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

// K workgroups: workgroup k finishes MSM k
__global__ void __launch_bounds__(256) k_msmv_finish(const Pt* __restrict__ partial, size_t nblocks, const int* __restrict__ bad, uint8_t* __restrict__ out /*K x 36*/,
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
// ---- resident point sets (sp_points, sp_msm_points, sp_msm_points_many): the same sum over points that do NOT change between calls — the two
// commitments of a ComputationCommitment, fixed for the lifetime of a circuit. The set is decoded once and keeps, per point, the multiples 1..8
// of 16^w P for all 64 windows (64 KiB a point), so a multiplication is a flat sum of table entries: no decode, no table build, no Horner
// doublings. K scalar vectors over the one set go through one launch chain, as above; sp_msm_points is the call with K = 1.
//   k_points_build   one lane per point, at upload: decode (flag word as above), then per window the table of the running base and base <- 16 base
//                    (points_fill); k_points_build_uniform: the same set from the generator stream's uniform bytes (sp_points_from_uniform: the
//                    verifier-only generators), the hash-to-curve map instead of the decode, the encoding written out;
//   k_msmp_digits    one lane per (MSM, scalar): out of Montgomery form, 64 signed digits, the [K][64][n] layout of k_msmv_prepare;
//   k_msmp_windows   k_msmv_windows with the lane's term fetched from window w's slice of the resident table, at the range's offset: a call
//                    multiplies n consecutive points of the set (sp_msm_points_range; the whole set is the range (0, count));
//   k_msmp_finish    K workgroups, one per MSM: 256 lanes stride over all 64 x nblocks partial sums (they carry their weight 16^w already),
//                    6 shuffle levels, the 4 wavefront sums through LDS, the encode on one lane; each writes its 32-byte slot of the host page.
// Point operations on the critical path: 8 + ceil(64 nblocks / 256) + 8 + the encode.
// the 64 window tables of point j of a set of n: per window the multiples 1..8 of the running base, then base <- 16 base
__device__ __forceinline__ void points_fill(Pt base, size_t j, size_t n, Pt* __restrict__ table /*[64][n][8]*/) {
#pragma unroll 1
  for (size_t w = 0; w < SP_VAR_WINDOWS; w++) {
    Pt T[SP_VAR_TABLE];
    pt_var_table(base, T);
    for (int m = 0; m < SP_VAR_TABLE; m++) table[(w * n + j) * SP_VAR_TABLE + m] = T[m];
    base = pt_dbl(T[SP_VAR_TABLE - 1]);  // 16 base = 2 (8 base)
  }
}
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
  points_fill(base, j, n, table);
}
// the same set from 64 uniform bytes a point (MultiCommitGens::new, commitments.rs:21-30: from_uniform_bytes, the map k_points_load of gens.hip
// runs in mode 1): one lane per point; the encoding goes out first, the tables are filled from the point the map produced
__global__ void __launch_bounds__(64) k_points_build_uniform(const uint8_t* __restrict__ uniform, size_t n, Pt* __restrict__ table /*[64][n][8]*/,
                                                             uint8_t* __restrict__ comp_out /*32 n*/) {
  const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  uint8_t b[64];
  for (int k = 0; k < 64; k++) b[k] = uniform[64 * j + k];
  const Pt base = pt_from_uniform_bytes(b);
  uint8_t c[32];
  pt_compress(base, c);
  for (int k = 0; k < 32; k++) comp_out[32 * j + k] = c[k];
  points_fill(base, j, n, table);
}

__global__ void __launch_bounds__(MV_BLOCK) k_msmp_digits(const Fq* __restrict__ S, unsigned n, unsigned total /* K n */, int8_t* __restrict__ digits /*[K][64][n]*/) { SP_FG_PRIO();
  const unsigned g = blockIdx.x * MV_BLOCK + threadIdx.x;
  if (g >= total) return;
  const unsigned k = g / n, j = g - k * n;
  int8_t d[SP_VAR_WINDOWS];
  fq_signed_digits4(fq_from_mont(ld_fq(S + g)), d);
  int8_t* dk = digits + (size_t)k * SP_VAR_WINDOWS * n;
  for (int w = 0; w < SP_VAR_WINDOWS; w++) dk[(size_t)w * n + j] = d[w];
}

// grid (nblocks, 64 windows, K): partial[(k * 64 + w) * nblocks + blk] = sum over the block's 256 terms of digit_w(S[k][j]) * 16^w P[off + j], j < n:
// the n points from `off` of a resident table of `stride` points a window (the whole set: off = 0, n = stride)
__global__ void __launch_bounds__(MV_BLOCK) k_msmp_windows(const Pt* __restrict__ table, size_t stride, size_t off, const int8_t* __restrict__ digits, size_t n,
                                                           Pt* __restrict__ partial) { SP_FG_PRIO();
  __shared__ Pt sm[MV_BLOCK / 64];
  const int t = threadIdx.x;
  const size_t w = blockIdx.y, k = blockIdx.z, j = (size_t)blockIdx.x * MV_BLOCK + t;
  Pt p = pt_identity();
  if (j < n) {
    const int d = digits[(k * SP_VAR_WINDOWS + w) * n + j];
    if (d != 0) {
      p = table[(w * stride + off + j) * SP_VAR_TABLE + ((d < 0 ? -d : d) - 1)];
      if (d < 0) p = pt_neg(p);
    }
  }
  msmv_block_sum(p, sm, &partial[(k * SP_VAR_WINDOWS + w) * gridDim.x + blockIdx.x]);
}

// K workgroups: workgroup k adds the nparts partial sums of MSM k
__global__ void __launch_bounds__(256) k_msmp_finish(const Pt* __restrict__ partial, size_t nparts, uint8_t* __restrict__ out /*K x 32*/, DoneSig sig) { SP_FG_PRIO();
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

// ---- row commitments of a DEVICE table over a range of a resident set (sp_commit_rows_points): out[r] = sum_j Z[r cols + j] P[off + j], the
// unblinded DensePolynomial::commit_inner of a verifier that holds a generator stream as a resident set and commits to a circuit itself. The
// table is as large as the prover's (4096 x 4096 scalars at 2^20), so nothing per scalar is written out: no digit array, no per-window grid.
//   k_rowp_sum      one lane per (row, column), a block per (row, slice of 256 columns), rows and slices flattened on gridDim.x: the scalar out
//                   of Montgomery form, its signed 4-bit digits recoded on the fly from the low end (fq_signed_digits4's carry chain over a
//                   shifted copy of the limbs: no runtime-indexed array), +-table entry added into the lane's accumulator for every non-zero
//                   digit, and the loop LEFT once what remains of the scalar and the carry are zero — an address or a timestamp of 20 bits costs
//                   5..6 additions, not 64, and rows of such scalars (12 of the 15 slots of SPARK's comb_ops) leave together. Then the block sum;
//   k_rowp_finish   one lane per row: the row's slices added up, the encode, 32 bytes into a device buffer the host fetches.
__global__ void __launch_bounds__(MV_BLOCK) k_rowp_sum(const Pt* __restrict__ table, size_t stride, size_t off, const Fq* __restrict__ Z, size_t cols, size_t nslices,
                                                       Pt* __restrict__ partial /*[rows][nslices]*/) {
  __shared__ Pt sm[MV_BLOCK / 64];
  const size_t b = blockIdx.x, row = b / nslices, j = (b - row * nslices) * MV_BLOCK + threadIdx.x;
  Pt acc = pt_identity();
  if (j < cols) {  // lanes past the row's end keep the identity: every lane reaches the block sum
    const Fq k = fq_from_mont(ld_fq(Z + row * cols + j));
    uint64_t l0 = k.l[0], l1 = k.l[1], l2 = k.l[2], l3 = k.l[3];
    const Pt* tp = table + (off + j) * SP_VAR_TABLE;  // window w of point off + j: tp + w stride 8
    int carry = 0;
#pragma unroll 1
    for (int w = 0; w < SP_VAR_WINDOWS && ((l0 | l1 | l2 | l3) != 0 || carry); w++) {  // k < q < 2^253: the last carry fits window 63
      const int v = (int)(l0 & 15) + carry;
      carry = v > 8;
      const int d = carry ? v - 16 : v;
      l0 = (l0 >> 4) | (l1 << 60); l1 = (l1 >> 4) | (l2 << 60); l2 = (l2 >> 4) | (l3 << 60); l3 >>= 4;
      if (d != 0) {
        Pt p = tp[(size_t)w * stride * SP_VAR_TABLE + ((d < 0 ? -d : d) - 1)];
        if (d < 0) p = pt_neg(p);
        acc = pt_add(acc, p);
      }
    }
  }
  msmv_block_sum(acc, sm, &partial[b]);
}
__global__ void __launch_bounds__(64) k_rowp_finish(const Pt* __restrict__ partial, size_t rows, size_t nslices, uint8_t* __restrict__ out /*32 rows*/) {
  const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  const Pt* part = partial + r * nslices;
  Pt acc = part[0];
#pragma unroll 1
  for (size_t s = 1; s < nslices; s++) acc = pt_add(acc, part[s]);
  uint8_t c[32];
  Pt10 r10 = pt10_load(acc);
  fe10_pin(r10.X); fe10_pin(r10.Y); fe10_pin(r10.Z); fe10_pin(r10.T);
  pt10_compress(r10, c);
  uint8_t* o = out + 32 * r;
  for (int i = 0; i < 32; i++) o[i] = c[i];
}

bool many_args_ok(size_t n, size_t K) { return n != 0 && K != 0 && n <= MV_MAX_N && K <= MVM_MAX_K && n * K <= MVM_MAX_TERMS; }

// the call's host inputs, back to back, where the kernels read them: the host-mapped page while they fit, else the device staging buffer
// (the pinned buffer is sized for the whole call first: the second copy must never regrow it under the first, whatever ensure_pinned's
// growth factor is)
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

// K multiplications over K x n points of the caller: status[k] is SP_OK or SP_EPOINT, out[k] is written where it is SP_OK. One round trip.
int32_t msm_var_run(sp_ctx* c, const uint8_t* points, const uint64_t* S, size_t n, size_t K, uint8_t* out, int32_t* status) {
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
    hipLaunchKernelGGL(k_msmv_prepare, dim3((unsigned)((nk + 63) / 64)), dim3(64), 0, c->stream, d_enc, (const Fq*)d_S, (unsigned)n, (unsigned)nk, table, digits, bad);
    hipLaunchKernelGGL(k_msmv_windows, dim3((unsigned)nblocks, SP_VAR_WINDOWS, (unsigned)K), dim3(MV_BLOCK), 0, c->stream, (const Pt*)table, (const int8_t*)digits, n,
                       partial);
    hipLaunchKernelGGL(k_msmv_finish, dim3((unsigned)K), dim3(256), 0, c->stream, (const Pt*)partial, nblocks, (const int*)bad, res, sig);
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

// K scalar vectors over the points [off, off + n) of the resident set pts (off + n <= pts->n, on c's device): out[k], always written. One round
// trip. Everything but the table fetch has the length of the range: the digits, the blocks, the partial sums and where the scalars are staged.
int32_t msm_points_run(sp_ctx* c, const sp_points* pts, size_t off, size_t n, const uint64_t* S, size_t K, uint8_t* out) {
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
    hipLaunchKernelGGL(k_msmp_digits, dim3((unsigned)((nk + MV_BLOCK - 1) / MV_BLOCK)), dim3(MV_BLOCK), 0, c->stream, (const Fq*)d_S, (unsigned)n, (unsigned)nk, digits);
    hipLaunchKernelGGL(k_msmp_windows, dim3((unsigned)nblocks, SP_VAR_WINDOWS, (unsigned)K), dim3(MV_BLOCK), 0, c->stream, (const Pt*)pts->table, pts->n, off, (const int8_t*)digits,
                       n, partial);
    hipLaunchKernelGGL(k_msmp_finish, dim3((unsigned)K), dim3(256), 0, c->stream, (const Pt*)partial, nparts, res, sig);
  }
  int32_t rc = sig_wait(c, sig);
  pool_release(c, buf, total);
  if (rc != SP_OK) return rc;
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  memcpy(out, res, 32 * K);
  return SP_OK;
}

// rows x cols scalars of a device table over the points [off, off + cols) of pts (arguments checked by the caller): out[r], 32 rows bytes through
// a device buffer (they do not fit the host result page). One launch chain, one round trip; no threshold but the slices of 256 columns.
int32_t commit_points_run(sp_ctx* c, const sp_points* pts, size_t off, const Fq* dZ, size_t rows, size_t cols, uint8_t* out) {
  HIPCHK(hipSetDevice(c->dev));
  const size_t nslices = (cols + MV_BLOCK - 1) / MV_BLOCK, nparts = rows * nslices;
  // device buffer: [partial rows x nslices Pt][32 rows bytes of encodings]
  const size_t off_out = nparts * sizeof(Pt), total = off_out + 32 * rows;
  void* buf = nullptr;
  SPCHK(pool_alloc(c, total, &buf));
  Pt* partial = (Pt*)buf;
  uint8_t* d_out = (uint8_t*)buf + off_out;
  {
    const double terms = (double)rows * (double)cols;
    ProfScope ps(c, PF_COMMIT_POINTS, 32.0 * terms + 32.0 * (double)rows, nullptr, (double)SP_VAR_WINDOWS * terms + (double)nparts);
    hipLaunchKernelGGL(k_rowp_sum, dim3((unsigned)nparts), dim3(MV_BLOCK), 0, c->stream, (const Pt*)pts->table, pts->n, off, dZ, cols, nslices, partial);
    hipLaunchKernelGGL(k_rowp_finish, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, c->stream, (const Pt*)partial, rows, nslices, d_out);
  }
  int32_t rc = hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;  // a refused launch: out is not written
  if (rc == SP_OK) rc = fetch_out(c, d_out, out, 32 * rows);
  pool_release(c, buf, total);
  return rc;
}
}  // namespace

extern "C" int32_t sp_msm_var(sp_ctx* c, const uint8_t* points, const uint64_t* S, size_t n, uint8_t out[32]) {
  if (!c || !points || !S || !out || n == 0 || n > MV_MAX_N) return SP_EINVAL;
  int32_t status = SP_OK;
  SPCHK(msm_var_run(c, points, S, n, 1, out, &status));
  return status;  // SP_EPOINT: out is not written
}
extern "C" int32_t sp_msm_var_many(sp_ctx* c, const uint8_t* points, const uint64_t* S, size_t n, size_t K, uint8_t* out, int32_t* status) {
  if (!c || !points || !S || !out || !status || !many_args_ok(n, K)) return SP_EINVAL;
  return msm_var_run(c, points, S, n, K, out, status);
}

namespace {
// a resident set of n points from their encodings (uniform == false: 32 bytes a point, decoded and checked) or from the generator stream's
// uniform bytes (64 a point: the set produces its encodings). One launch, one lane per point; the set keeps the encodings on the host too.
int32_t points_make(sp_ctx* c, const uint8_t* in, bool uniform, size_t n, uint8_t* compressed_out, sp_points** out) {
  if (!c || !in || !out || n == 0 || n > MV_MAX_N) return SP_EINVAL;
  *out = nullptr;
  HIPCHK(hipSetDevice(c->dev));
  const size_t in_bytes = (uniform ? 64 : 32) * n;
  SPCHK(ensure_dstage(c, in_bytes));
  SPCHK(stage_in(c, 0, in, in_bytes));
  const size_t table_bytes = n * SP_VAR_WINDOWS * SP_VAR_TABLE * sizeof(Pt), comp_bytes = uniform ? (32 * n + 255) & ~(size_t)255 : 0;
  uint8_t* buf = nullptr;  // the table, then (uniform) the encodings the kernel writes, then the flag word
  HIPCHK(hipMalloc((void**)&buf, table_bytes + comp_bytes + 256));
  uint8_t* d_comp = buf + table_bytes;
  int* bad = (int*)(buf + table_bytes + comp_bytes);
  int flag = 0;
  std::vector<uint8_t> comp;
  int32_t rc = SP_OK;
  try {
    if (uniform) comp.resize(32 * n);
    else comp.assign(in, in + 32 * n);
  } catch (const std::bad_alloc&) {
    rc = SP_ENOMEM;
  }
  if (rc == SP_OK && !uniform) rc = hipMemsetAsync(bad, 0, 4, c->stream) == hipSuccess ? SP_OK : SP_EHIP;
  if (rc == SP_OK) {
    const dim3 grid((unsigned)((n + 63) / 64));
    if (uniform) hipLaunchKernelGGL(k_points_build_uniform, grid, dim3(64), 0, c->stream, (const uint8_t*)c->dstage, n, (Pt*)buf, d_comp);
    else hipLaunchKernelGGL(k_points_build, grid, dim3(64), 0, c->stream, (const uint8_t*)c->dstage, n, (Pt*)buf, bad);
    rc = uniform ? fetch_out(c, d_comp, comp.data(), 32 * n) : fetch_out(c, bad, &flag, 4);
  }
  if (rc == SP_OK && hipGetLastError() != hipSuccess) rc = SP_EHIP;
  if (rc == SP_OK && flag) rc = SP_EPOINT;
  sp_points* p = rc == SP_OK ? new (std::nothrow) sp_points{c->dev, n, (Pt*)buf, {}} : nullptr;
  if (!p) {
    (void)hipFree(buf);
    return rc == SP_OK ? SP_ENOMEM : rc;
  }
  if (uniform && compressed_out) memcpy(compressed_out, comp.data(), 32 * n);
  p->comp = std::move(comp);
  *out = p;
  return SP_OK;
}
bool range_ok(const sp_points* pts, size_t off, size_t n) { return n != 0 && off <= pts->n && n <= pts->n - off; }
}  // namespace

extern "C" int32_t sp_points_upload(sp_ctx* c, const uint8_t* compressed, size_t n, sp_points** out) { return points_make(c, compressed, false, n, nullptr, out); }
extern "C" int32_t sp_points_from_uniform(sp_ctx* c, const uint8_t* uniform, size_t n, uint8_t* compressed_out, sp_points** out) {
  return points_make(c, uniform, true, n, compressed_out, out);
}
extern "C" void sp_points_free(sp_points* p) {
  if (!p) return;
  host_commit_forget(p);  // the host window tables of its few-term commitments (host_commit.hip)
  (void)hipSetDevice(p->dev);
  (void)hipFree(p->table);  // waits for whatever still reads the table
  delete p;
}
extern "C" size_t sp_points_count(const sp_points* p) { return p ? p->n : 0; }
extern "C" size_t sp_points_table_bytes(const sp_points* p) { return p ? p->n * SP_VAR_WINDOWS * SP_VAR_TABLE * sizeof(Pt) : 0; }

// one launch path: the whole-set calls are the (0, count) range
extern "C" int32_t sp_msm_points_range(sp_ctx* c, const sp_points* pts, size_t off, size_t n, const uint64_t* S, uint8_t out[32]) {
  if (!c || !pts || !S || !out || !range_ok(pts, off, n) || pts->dev != c->dev) return SP_EINVAL;
  return msm_points_run(c, pts, off, n, S, 1, out);
}
extern "C" int32_t sp_msm_points_range_many(sp_ctx* c, const sp_points* pts, size_t off, size_t n, const uint64_t* S, size_t K, uint8_t* out) {
  if (!c || !pts || !S || !out || !many_args_ok(n, K) || !range_ok(pts, off, n) || pts->dev != c->dev) return SP_EINVAL;
  return msm_points_run(c, pts, off, n, S, K, out);
}
extern "C" int32_t sp_msm_points(sp_ctx* c, const sp_points* pts, const uint64_t* S, size_t n, uint8_t out[32]) {
  if (!pts || n != pts->n) return SP_EINVAL;
  return sp_msm_points_range(c, pts, 0, n, S, out);
}
extern "C" int32_t sp_msm_points_many(sp_ctx* c, const sp_points* pts, const uint64_t* S, size_t n, size_t K, uint8_t* out) {
  if (!pts || n != pts->n) return SP_EINVAL;
  return sp_msm_points_range_many(c, pts, 0, n, S, K, out);
}
extern "C" int32_t sp_commit_rows_points(sp_ctx* c, const sp_points* pts, size_t off, const sp_table* Z, size_t z_off, size_t rows, size_t cols, uint8_t* out) {
  constexpr size_t MAX_ROWS = 65536;
  if (!c || !pts || !Z || !out || rows == 0 || rows > MAX_ROWS || !range_ok(pts, off, cols)) return SP_EINVAL;
  // cols <= 65536 (the set's size) and rows <= 65536: rows * cols does not wrap
  if (z_off > Z->len || rows * cols > Z->len - z_off || pts->dev != c->dev || !Z->ctx || Z->ctx->dev != c->dev) return SP_EINVAL;
  return commit_points_run(c, pts, off, Z->d + z_off, rows, cols, out);
}
