// spartan_amd: R1CSInstance::evaluate (r1cs.rs:300-303) of up to four resident matrices at K points (rx_k, ry_k) in ONE pass over the entries
// (sp_sparse_evaluate_many_begin): what K NIZK verifications of one circuit ask for when they advance in lock step (verifier.cc,
// NIZK::verify_many). K calls of sp_eq_expand x 2 + sp_sparse_evaluate_begin would build 2 K full chi tables (96 MiB a pair at 2^20) and read
// every entry K times. Here no full table exists: chi(r)[i] = chi(r_hi)[i >> lo] * chi(r_lo)[i & (2^lo - 1)], hi = ell - ell/2, lo = ell/2 (the
// identity k_eq_outer of fq_ops.hip is built on), and only the HALF tables are built, at most 2^16 entries each, one pair per proof and
// side, stored proof-minor (half[j * K + k]) so that the K proofs of an entry read K consecutive scalars.
//   k_eq_half_many     the 4+4 product form of k_eq_expand_small with the proof on grid.y and the table (x hi, x lo, y hi, y lo) on grid.z;
//   k_sparse_eval_kp   lanes are (entry, proof), proof minor, K padded to Kp in {1, 2, 4, .., 64}: a wavefront covers 64 / Kp entries, the lanes
//                      of an entry load its row, col and val from one address (one fetch, broadcast) and form hi_x lo_x hi_y lo_y val with four
//                      multiplications; per-proof sums over a grid-stride loop, added across the lanes of a proof (shuffles at strides >= Kp,
//                      then LDS across the four wavefronts) into partials[m][blk][k]; the matrix is on grid.y as in k_sparse_eval_many;
//   k_sparse_many_sums one block per matrix adds the partials, out[k * count + m].
// Memory of a call: the half tables (32 K (2^hi_x + 2^lo_x + 2^hi_y + 2^lo_y) bytes: ~10 MB at 2^20 x 2^21 with K = 64) plus the partials
// (32 count K blocks, blocks <= EM_MAX_BLOCKS). NOTHING in a call is proportional to K (num_rows + num_cols).
// Field arithmetic is exact: the product of the same factors in another order is the same element, hence the same canonical limbs as
// sp_eq_expand x 2 + sp_sparse_evaluate give for that proof.
#include "internal.hpp"

namespace {
constexpr size_t EM_MAX_K = SP_EVAL_MANY_MAX_K;
constexpr size_t EM_MAX_BLOCKS = 1024;  // cap of the partials grid (blocks per matrix)
constexpr size_t EM_MAX_ELL = 32;       // as sp_eq_expand: a half has at most 16 variables
constexpr size_t EM_R_BYTES = 32 * 2 * EM_MAX_ELL * EM_MAX_K;  // the challenge vectors of a full batch (128 KiB)
static_assert(EM_MAX_K == 64, "a proof's lanes lie in one wavefront: Kp <= 64");

struct EqHalves {
  const Fq* r[4];  // proof k's variables of table z start at r[z] + k * stride
  Fq* out[4];
  unsigned ell[4];  // 0..16
  unsigned stride;  // scalars between two proofs' challenge vectors
};
// k_eq_expand_small (fq_ops.hip) for K proofs and four tables at once: block (x, k, z) builds entries [256 x, 256 x + 256) of chi(r_z of proof k)
// and stores entry i at out[z][i * K + k]. ell = 0 (the low half of a one-variable point) is the one-entry table {1}.
__global__ void __launch_bounds__(256) k_eq_half_many(EqHalves H, unsigned K) { SP_FG_PRIO();
  __shared__ Fq r[16];
  __shared__ Fq ta[16], tb[16];
  __shared__ Fq hi;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const unsigned k = blockIdx.y, z = blockIdx.z;
  const int ell = (int)H.ell[z];
  if (((size_t)blockIdx.x * 256) >> ell) return;  // the whole block: this table is shorter than the longest of the four
  if (t < ell) r[t] = ld_fq(H.r[z] + (size_t)k * H.stride + t);
  __syncthreads();
  const int nlo = ell < 8 ? ell : 8, nb = nlo / 2, na = nlo - nb, nhi = ell - nlo;
  auto factor = [&](int v, bool bit) {  // chi factor of variable v: r[v] or 1 - r[v]
    Fq rv = r[v], f = fq_sub(fq_one(), rv);
#pragma unroll
    for (int w = 0; w < 4; w++) f.l[w] = bit ? rv.l[w] : f.l[w];
    return f;
  };
  if (wave == 0 && lane < 16) {
    Fq acc = fq_one();
    if (lane < (1 << na))
      for (int v = 0; v < na; v++) { Fq f = factor(nhi + v, (lane >> (na - 1 - v)) & 1); acc = v ? fq_mul(acc, f) : f; }
    ta[lane] = acc;
  } else if (wave == 1 && lane < 16) {
    Fq acc = fq_one();
    if (lane < (1 << nb))
      for (int v = 0; v < nb; v++) { Fq f = factor(nhi + na + v, (lane >> (nb - 1 - v)) & 1); acc = v ? fq_mul(acc, f) : f; }
    tb[lane] = acc;
  } else if (wave == 2 && lane == 0) {
    Fq acc = fq_one();
    for (int v = 0; v < nhi; v++) { Fq f = factor(v, (blockIdx.x >> (nhi - 1 - v)) & 1); acc = v ? fq_mul(acc, f) : f; }
    hi = acc;
  }
  __syncthreads();
  if (nhi > 0 && t < (1 << na)) ta[t] = fq_mul(ta[t], hi);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + t;
  if (i >> ell) return;
  Fq v = ta[(t >> nb) & ((1 << na) - 1)];
  if (nb > 0) v = fq_mul(v, tb[t & ((1 << nb) - 1)]);
  st_fq(H.out[z] + i * K + k, v);
}

struct EvalManyArgs {
  const uint32_t *row[4], *col[4];
  const Fq* val[4];
  size_t nnz[4];
  const Fq *xh, *xl, *yh, *yl;  // half tables, proof-minor
  unsigned lo_x, lo_y;
  unsigned K, lg_kp;
};
// grid (blocks, matrices). Thread g of the launch is proof g & (Kp - 1) of entry g >> lg Kp (256 is a multiple of Kp: the proof of a thread is
// that of its lane). Row and column indices are below num_rows <= 2^ell_x and num_cols <= 2^ell_y (checked at upload and by the caller), so every
// half-table index is inside its table. partials[(m * gridDim.x + blk) * K + k]
__global__ void __launch_bounds__(256) k_sparse_eval_kp(EvalManyArgs A, Fq* __restrict__ partials) { SP_FG_PRIO();
  __shared__ Fq sm[4][64];
  const int m = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const unsigned K = A.K, lg = A.lg_kp, kp = 1u << lg, k = (unsigned)t & (kp - 1);
  const uint32_t* __restrict__ row = A.row[m];
  const uint32_t* __restrict__ col = A.col[m];
  const Fq* __restrict__ val = A.val[m];
  const size_t nnz = A.nnz[m], step = ((size_t)gridDim.x * 256) >> lg;
  const uint32_t mask_x = (1u << A.lo_x) - 1, mask_y = (1u << A.lo_y) - 1;
  Fq acc = fq_zero();
  if (k < K)  // the padding lanes read nothing and add zero
    for (size_t e = ((size_t)blockIdx.x * 256 + t) >> lg; e < nnz; e += step) {
      const uint32_t r = row[e], c = col[e];
      const Fq x = fq_mul(ld_fq(A.xh + (size_t)(r >> A.lo_x) * K + k), ld_fq(A.xl + (size_t)(r & mask_x) * K + k));
      const Fq y = fq_mul(ld_fq(A.yh + (size_t)(c >> A.lo_y) * K + k), ld_fq(A.yl + (size_t)(c & mask_y) * K + k));
      acc = fq_add(acc, fq_mul(fq_mul(x, y), ld_fq(val + e)));
    }
  for (unsigned s = 32; s >= kp; s >>= 1) {  // across the lanes of the wavefront that share the proof (kp = 64: none)
    Fq o;
#pragma unroll
    for (int w = 0; w < 4; w++) o.l[w] = __shfl_xor((unsigned long long)acc.l[w], (int)s, 64);
    acc = fq_add(acc, o);
  }
  if ((unsigned)lane < kp) sm[wave][lane] = acc;
  __syncthreads();
  if ((unsigned)t < K) {
    Fq s = fq_add(fq_add(sm[0][t], sm[1][t]), fq_add(sm[2][t], sm[3][t]));
    st_fq(partials + ((size_t)m * gridDim.x + blockIdx.x) * K + t, s);
  }
}
// one block per matrix: out[k * count + m] = sum over blk of partials[(m * nblk + blk) * K + k]. Thread t adds the blocks t >> lg Kp, + 256 / Kp, ..
// of proof t & (Kp - 1); the tree below only joins threads of one proof (every stride is a multiple of Kp).
__global__ void __launch_bounds__(256) k_sparse_many_sums(const Fq* __restrict__ partials, size_t nblk, unsigned K, unsigned lg_kp, unsigned count,
                                                          Fq* __restrict__ out) { SP_FG_PRIO();
  __shared__ Fq sm[256];
  const unsigned t = threadIdx.x, kp = 1u << lg_kp, k = t & (kp - 1), m = blockIdx.x;
  Fq acc = fq_zero();
  if (k < K)
    for (size_t b = t >> lg_kp; b < nblk; b += 256u >> lg_kp) acc = fq_add(acc, ld_fq(partials + ((size_t)m * nblk + b) * K + k));
  sm[t] = acc;
  __syncthreads();
  for (unsigned s = 128; s >= kp; s >>= 1) {
    if (t < s) sm[t] = fq_add(sm[t], sm[t + s]);
    __syncthreads();
  }
  if (t < K) st_fq(out + (size_t)t * count + m, sm[t]);
}
}  // namespace

// The K challenge vectors reach the device through a pinned page of the context's own (em_pinned): the call does not wait, so neither the
// host-mapped page's general area nor the shared staging buffer may hold them — the next call on the context overwrites both at once, while
// this job's kernels still wait on the low-priority stream. k_eq_half_many reads the page in place; em_ev fires when it has, and the next
// batched evaluation waits for that before it writes its own vectors.
extern "C" int32_t sp_sparse_evaluate_many_begin(sp_ctx* c, const sp_sparse* const* ms, size_t count, const uint64_t* rx, size_t ell_x, const uint64_t* ry,
                                                 size_t ell_y, size_t K, sp_job** out) {
  if (!c || !ms || !rx || !ry || !out || count == 0 || count > 4 || K == 0 || K > EM_MAX_K || ell_x == 0 || ell_x > EM_MAX_ELL || ell_y == 0 ||
      ell_y > EM_MAX_ELL)
    return SP_EINVAL;
  EvalManyArgs A;
  memset(&A, 0, sizeof A);
  size_t max_nnz = 1;
  double bytes = 0, ents = 0;
  for (size_t m = 0; m < count; m++) {
    if (!ms[m] || ms[m]->num_rows > ((size_t)1 << ell_x) || ms[m]->num_cols > ((size_t)1 << ell_y)) return SP_EINVAL;
    A.row[m] = ms[m]->csr_row; A.col[m] = ms[m]->csr_col; A.val[m] = ms[m]->csr_val; A.nnz[m] = ms[m]->nnz;
    if (ms[m]->nnz > max_nnz) max_nnz = ms[m]->nnz;
    ents += (double)ms[m]->nnz;
    bytes += (double)ms[m]->nnz * (8 + 32 + 128.0 * (double)K);  // an entry once, four half-table scalars per proof
  }
  HIPCHK(hipSetDevice(c->dev));
  if (!c->stream_low) return SP_EHIP;
  unsigned lg_kp = 0;
  while (((size_t)1 << lg_kp) < K) lg_kp++;
  const size_t lo_x = ell_x / 2, hi_x = ell_x - lo_x, lo_y = ell_y / 2, hi_y = ell_y - lo_y;
  const size_t n_half[4] = {(size_t)1 << hi_x, (size_t)1 << lo_x, (size_t)1 << hi_y, (size_t)1 << lo_y};
  const size_t ell_half[4] = {hi_x, lo_x, hi_y, lo_y};
  const size_t nblk = grid_for(max_nnz << lg_kp, EM_MAX_BLOCKS);  // 256 >> lg_kp entries a block and pass
  // the job's buffer: [x hi | x lo | y hi | y lo] K entries each, [partials count x nblk x K], [out K x count]
  size_t off_half[4], off = 0;
  for (int z = 0; z < 4; z++) { off_half[z] = off; off += 32 * K * n_half[z]; }
  const size_t off_part = off, off_out = off_part + 32 * count * nblk * K;
  if (!c->em_pinned) {
    HIPCHK(hipHostMalloc((void**)&c->em_pinned, EM_R_BYTES, hipHostMallocDefault));
    if (hipEventCreateWithFlags(&c->em_ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(c->em_pinned); c->em_pinned = nullptr; c->em_ev = nullptr; return SP_EHIP; }
  } else {
    HIPCHK(hipEventSynchronize(c->em_ev));  // the previous batch's kernel has read its vectors
  }
  sp_job* j = new (std::nothrow) sp_job();
  if (!j) return SP_ENOMEM;
  j->ctx = c; j->rows = count * K; j->stream = c->stream_low; j->scratch = nullptr;
  j->out_off = off_out;
  j->scratch_bytes = off_out + 32 * count * K;
  int32_t rc = pool_alloc(c, j->scratch_bytes, (void**)&j->scratch);
  if (rc != SP_OK) { delete j; return rc; }
  hipEvent_t ready;
  if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&j->done, hipEventDisableTiming) != hipSuccess) {
    pool_release(c, j->scratch, j->scratch_bytes); delete j; return SP_EHIP;
  }
  // proof k's vectors side by side: [rx_k | ry_k], ell_x + ell_y scalars
  const size_t stride = ell_x + ell_y;
  for (size_t k = 0; k < K; k++) {
    memcpy(c->em_pinned + 32 * stride * k, rx + 4 * ell_x * k, 32 * ell_x);
    memcpy(c->em_pinned + 32 * (stride * k + ell_x), ry + 4 * ell_y * k, 32 * ell_y);
  }
  EqHalves H;
  const Fq* r0 = (const Fq*)c->em_pinned;
  const Fq* r_src[4] = {r0, r0 + hi_x, r0 + ell_x, r0 + ell_x + hi_y};
  size_t longest = 0;
  for (int z = 0; z < 4; z++) {
    H.r[z] = r_src[z]; H.out[z] = (Fq*)(j->scratch + off_half[z]); H.ell[z] = (unsigned)ell_half[z];
    if (n_half[z] > longest) longest = n_half[z];
  }
  H.stride = (unsigned)stride;
  A.xh = H.out[0]; A.xl = H.out[1]; A.yh = H.out[2]; A.yl = H.out[3];
  A.lo_x = (unsigned)lo_x; A.lo_y = (unsigned)lo_y; A.K = (unsigned)K; A.lg_kp = lg_kp;
  (void)hipEventRecord(ready, c->stream);  // the buffer came from the main stream's pool: behind what is queued there
  (void)hipStreamWaitEvent(c->stream_low, ready, 0);
  {
    ProfScope ps(c, PF_SPARSE, bytes, c->stream_low, 4.0 * (double)K * ents);
    hipLaunchKernelGGL(k_eq_half_many, dim3((unsigned)((longest + 255) / 256), (unsigned)K, 4), dim3(256), 0, c->stream_low, H, (unsigned)K);
    (void)hipEventRecord(c->em_ev, c->stream_low);
    hipLaunchKernelGGL(k_sparse_eval_kp, dim3((unsigned)nblk, (unsigned)count), dim3(256), 0, c->stream_low, A, (Fq*)(j->scratch + off_part));
    hipLaunchKernelGGL(k_sparse_many_sums, dim3((unsigned)count), dim3(256), 0, c->stream_low, (const Fq*)(j->scratch + off_part), nblk, (unsigned)K, lg_kp,
                       (unsigned)count, (Fq*)(j->scratch + off_out));
  }
  (void)hipEventRecord(j->done, c->stream_low);
  (void)hipEventDestroy(ready);
  if (hipGetLastError() != hipSuccess) {
    (void)hipStreamSynchronize(c->stream_low);
    (void)hipEventDestroy(j->done); pool_release(c, j->scratch, j->scratch_bytes); delete j; return SP_EHIP;
  }
  *out = j;
  return SP_OK;
}
