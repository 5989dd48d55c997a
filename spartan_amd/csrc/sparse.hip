// spartan_amd: sparse R1CS matrices on the device (SparseMatPolynomial, src/sparse_mlpoly.rs:19-38).
// F_q has no atomic add, so both products are formulated as gathers over a row-sorted (CSR) and a
// column-sorted (CSC) copy built once at upload (instance setup, outside SNARK::prove).
#include <algorithm>
#include <numeric>

#include "internal.hpp"

// multiply_vec (sparse_mlpoly.rs:454-464)
__global__ void __launch_bounds__(256) k_spmv(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const Fq* __restrict__ val,
                                              const Fq* __restrict__ z, size_t num_rows, Fq* __restrict__ out) { SP_FG_PRIO();
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rows) return;
  Fq acc = fq_zero();
  for (uint32_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) acc = fq_add(acc, fq_mul(ld_fq(val + e), ld_fq(z + col[e])));
  st_fq(out + r, acc);
}

// ---- R1CSShape::is_sat (r1cs.rs:240-266): (A z)[r] * (B z)[r] == (C z)[r] for every row, fused — no Az, Bz, Cz tables are written ----
// A row of up to CHK_LANE_MAX entries is walked by one lane (the synthetic instance: one entry per row and matrix). A lane that walks a row
// keeps the other 63 lanes of its wavefront waiting, so a wavefront takes as long as its longest row: past 32 entries the 64 lanes do more
// reading the row side by side (coalesced col / val, 16 entries per lane and chunk) than one lane does alone, chunk launch included. A longer
// row is therefore cut into chunks of CHK_CHUNK entries that k_r1cs_chunks sums one wavefront each, whatever the row's length; k_r1cs_check
// adds a row's chunk sums across the lanes of the wavefront that owns the row (one partial per 65536 entries and lane).
constexpr uint32_t CHK_LANE_MAX = 32, CHK_CHUNK = 1024;
struct Csr3 {
  const uint32_t *row_ptr[3], *col[3];
  const Fq* val[3];
  const uint32_t *long_rows[3], *long_first[3], *chunk_beg[3], *chunk_end[3];
  uint32_t n_long[3], n_chunks[3], part_off[3];  // part_off: where a matrix's chunk sums start in `partials`
};
__device__ __forceinline__ Fq wave_sum_fq(Fq v) {  // the sum over the 64 lanes, in every lane
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    Fq o;
#pragma unroll
    for (int w = 0; w < 4; w++) o.l[w] = __shfl_xor((unsigned long long)v.l[w], m, 64);
    v = fq_add(v, o);
  }
  return v;
}
// grid (ceil(max chunks / 4), 3 matrices): one wavefront per chunk, partials[part_off[m] + k] = sum of val * z[col] over chunk k of matrix m
__global__ void __launch_bounds__(256) k_r1cs_chunks(Csr3 M, const Fq* __restrict__ z, Fq* __restrict__ partials) { SP_FG_PRIO();
  const int m = blockIdx.y;
  const unsigned lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= M.n_chunks[m]) return;  // the whole wavefront
  const uint32_t* __restrict__ col = M.col[m];
  const Fq* __restrict__ val = M.val[m];
  const uint32_t end = M.chunk_end[m][k];
  Fq acc = fq_zero();
  for (uint32_t e = M.chunk_beg[m][k] + lane; e < end; e += 64) acc = fq_add(acc, fq_mul(ld_fq(val + e), ld_fq(z + col[e])));
  acc = wave_sum_fq(acc);
  if (lane == 0) st_fq(partials + M.part_off[m] + k, acc);
}
// A wavefront owns 64 consecutive rows, a lane one of them. res[0] += violated rows, res[1] = min(res[1], first violated row),
// bitmap[r / 64] bit r % 64 = row r is violated (every word of ceil(num_rows / 64) is written).
__global__ void __launch_bounds__(256) k_r1cs_check(Csr3 M, const Fq* __restrict__ z, const Fq* __restrict__ partials, size_t num_rows,
                                                    unsigned long long* __restrict__ res, unsigned long long* __restrict__ bitmap) { SP_FG_PRIO();
  const unsigned lane = threadIdx.x & 63;
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t base = r - lane;  // first row of the wavefront
  if (base >= num_rows) return;
  const bool live = r < num_rows;
  uint32_t beg[3], len[3];
  bool is_long = false;
#pragma unroll
  for (int m = 0; m < 3; m++) {
    beg[m] = live ? M.row_ptr[m][r] : 0;
    len[m] = live ? M.row_ptr[m][r + 1] - beg[m] : 0;
    is_long |= len[m] > CHK_LANE_MAX;
  }
  Fq s[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    s[m] = fq_zero();
    if (!is_long)
      for (uint32_t e = beg[m]; e < beg[m] + len[m]; e++) s[m] = fq_add(s[m], fq_mul(ld_fq(M.val[m] + e), ld_fq(z + M.col[m][e])));
  }
  // rows with a long side: the wavefront takes them one by one (the loop is uniform), every matrix summed across the lanes
  for (unsigned long long todo = __ballot(is_long); todo; todo &= todo - 1) {
    const int src = __ffsll(todo) - 1;
    const uint32_t row = (uint32_t)(base + src);
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const uint32_t b = __shfl(beg[m], src, 64), n = __shfl(len[m], src, 64);
      Fq acc = fq_zero();
      if (n > CHK_LANE_MAX) {  // its chunk sums: `row` is in the ascending list of this matrix's long rows
        uint32_t lo = 0, hi = M.n_long[m];
        while (lo + 1 < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (M.long_rows[m][mid] <= row) lo = mid; else hi = mid;
        }
        const uint32_t k1 = M.long_first[m][lo + 1];
        for (uint32_t k = M.long_first[m][lo] + lane; k < k1; k += 64) acc = fq_add(acc, ld_fq(partials + M.part_off[m] + k));
      } else if (lane < n) {
        acc = fq_mul(ld_fq(M.val[m] + b + lane), ld_fq(z + M.col[m][b + lane]));
      }
      acc = wave_sum_fq(acc);
      if ((int)lane == src) s[m] = acc;
    }
  }
  const bool bad = live && !fq_eq(fq_mul(s[0], s[1]), s[2]);  // canonical limbs: equality of values is equality of limbs
  const unsigned long long mask = __ballot(bad);
  if (lane == 0) {
    bitmap[base >> 6] = mask;
    if (mask) {
      atomicAdd(res, (unsigned long long)__popcll(mask));
      atomicMin(res + 1, (unsigned long long)(base + (__ffsll(mask) - 1)));
    }
  }
}
struct Csc3 {
  const uint32_t* col_ptr[3];
  const uint32_t* row[3];
  const Fq* val[3];
  Fq w[3];
  int nm;
};
// compute_eval_table_sparse (sparse_mlpoly.rs:466-481) x nm, combined with weights (r1csproof.rs:275-283)
__global__ void __launch_bounds__(256) k_eval_table(Csc3 M, const Fq* __restrict__ rx, size_t num_cols, Fq* __restrict__ out) { SP_FG_PRIO();
  size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= num_cols) return;
  Fq tot = fq_zero();
  for (int k = 0; k < M.nm; k++) {
    Fq acc = fq_zero();
    for (uint32_t e = M.col_ptr[k][c]; e < M.col_ptr[k][c + 1]; e++) acc = fq_add(acc, fq_mul(ld_fq(rx + M.row[k][e]), ld_fq(M.val[k] + e)));
    tot = fq_add(tot, fq_mul(M.w[k], acc));
  }
  st_fq(out + c, tot);
}
// evaluate_with_tables (sparse_mlpoly.rs:429-438)
__global__ void __launch_bounds__(256) k_sparse_eval(const uint32_t* __restrict__ row, const uint32_t* __restrict__ col, const Fq* __restrict__ val,
                                                     size_t nnz, const Fq* __restrict__ tx, const Fq* __restrict__ ty, Fq* __restrict__ partials) { SP_FG_PRIO();
  __shared__ Fq sm[256];
  Fq acc[1] = {fq_zero()};
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (size_t)gridDim.x * blockDim.x)
    acc[0] = fq_add(acc[0], fq_mul(fq_mul(ld_fq(tx + row[e]), ld_fq(ty + col[e])), ld_fq(val + e)));
  block_sum_fq<1>(acc, sm);
  if (threadIdx.x == 0) st_fq(partials + blockIdx.x, acc[0]);
}

// several matrices in one launch (grid.y = matrix): partials[m * gridDim.x + blk]
struct SparseMany {
  const uint32_t *row[4], *col[4];
  const Fq* val[4];
  size_t nnz[4];
};
__global__ void __launch_bounds__(256) k_sparse_eval_many(SparseMany M, const Fq* __restrict__ tx, const Fq* __restrict__ ty, Fq* __restrict__ partials) { SP_FG_PRIO();
  __shared__ Fq sm[256];
  const int m = blockIdx.y;
  const uint32_t* __restrict__ row = M.row[m];
  const uint32_t* __restrict__ col = M.col[m];
  const Fq* __restrict__ val = M.val[m];
  Fq acc[1] = {fq_zero()};
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < M.nnz[m]; e += (size_t)gridDim.x * blockDim.x)
    acc[0] = fq_add(acc[0], fq_mul(fq_mul(ld_fq(tx + row[e]), ld_fq(ty + col[e])), ld_fq(val + e)));
  block_sum_fq<1>(acc, sm);
  if (threadIdx.x == 0) st_fq(partials + (size_t)m * gridDim.x + blockIdx.x, acc[0]);
}
__global__ void __launch_bounds__(256) k_sparse_sums(const Fq* __restrict__ partials, size_t nblk, Fq* __restrict__ out) { SP_FG_PRIO();  // block per matrix
  __shared__ Fq sm[256];
  Fq acc[1] = {fq_zero()};
  for (size_t b = threadIdx.x; b < nblk; b += 256) acc[0] = fq_add(acc[0], ld_fq(partials + (size_t)blockIdx.x * nblk + b));
  block_sum_fq<1>(acc, sm);
  if (threadIdx.x == 0) st_fq(out + blockIdx.x, acc[0]);
}

template <typename T>
static int32_t dev_put(sp_ctx* c, T** d, const std::vector<T>& h) {
  size_t bytes = sizeof(T) * (h.size() ? h.size() : 1);
  HIPCHK(hipMalloc((void**)d, bytes));
  if (!h.empty()) HIPCHK(hipMemcpy(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  return SP_OK;
}

// The long rows of a matrix and their chunks, from its row_ptr (device), once per matrix: a matrix without long rows gets no lists.
static int32_t check_plan(sp_ctx* c, const sp_sparse* m) {
  if (m->chk_built) return SP_OK;
  std::vector<uint32_t> ptr(m->num_rows + 1), rows, first, cb, ce;
  HIPCHK(hipMemcpy(ptr.data(), m->row_ptr, 4 * ptr.size(), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < m->num_rows; r++) {
    if (ptr[r + 1] - ptr[r] <= CHK_LANE_MAX) continue;
    rows.push_back((uint32_t)r);
    first.push_back((uint32_t)cb.size());
    for (uint64_t b = ptr[r]; b < ptr[r + 1]; b += CHK_CHUNK) { cb.push_back((uint32_t)b); ce.push_back((uint32_t)std::min<uint64_t>(b + CHK_CHUNK, ptr[r + 1])); }
  }
  if (!rows.empty()) {
    first.push_back((uint32_t)cb.size());
    SPCHK(dev_put(c, &m->chk_rows, rows));
    SPCHK(dev_put(c, &m->chk_first, first));
    SPCHK(dev_put(c, &m->chk_beg, cb));
    SPCHK(dev_put(c, &m->chk_end, ce));
  }
  m->chk_nrows = (uint32_t)rows.size(); m->chk_nchunks = (uint32_t)cb.size();
  m->chk_built = true;
  return SP_OK;
}

extern "C" {

int32_t sp_sparse_upload(sp_ctx* c, const uint64_t* rows, const uint64_t* cols, const uint64_t* vals, size_t nnz, size_t num_rows,
                         size_t num_cols, sp_sparse** out) {
  if (!c || !out || (nnz && (!rows || !cols || !vals)) || num_rows == 0 || num_cols == 0 || nnz >= 0xffffffffu) return SP_EINVAL;
  for (size_t i = 0; i < nnz; i++)
    if (rows[i] >= num_rows || cols[i] >= num_cols) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  sp_sparse* m = new (std::nothrow) sp_sparse();
  if (!m) return SP_ENOMEM;
  memset(m, 0, sizeof *m);
  m->ctx = c; m->nnz = nnz; m->num_rows = num_rows; m->num_cols = num_cols;
  const Fq* v = (const Fq*)vals;
  auto build = [&](const uint64_t* key, size_t nkeys, const uint64_t* other, std::vector<uint32_t>& ptr, std::vector<uint32_t>& oth,
                   std::vector<uint32_t>& keys_sorted, std::vector<Fq>& vv) {
    ptr.assign(nkeys + 1, 0);
    for (size_t i = 0; i < nnz; i++) ptr[key[i] + 1]++;
    for (size_t k = 0; k < nkeys; k++) ptr[k + 1] += ptr[k];
    std::vector<uint32_t> cur(ptr.begin(), ptr.end() - 1);
    oth.resize(nnz); vv.resize(nnz); keys_sorted.resize(nnz);
    for (size_t i = 0; i < nnz; i++) {  // stable: preserves the entry order within a key
      uint32_t pos = cur[key[i]]++;
      oth[pos] = (uint32_t)other[i];
      keys_sorted[pos] = (uint32_t)key[i];
      vv[pos] = v[i];
    }
  };
  std::vector<uint32_t> ptr, oth, ks;
  std::vector<Fq> vv;
  int32_t rc;
  build(rows, num_rows, cols, ptr, oth, ks, vv);
  if ((rc = dev_put(c, &m->row_ptr, ptr)) || (rc = dev_put(c, &m->csr_col, oth)) || (rc = dev_put(c, &m->csr_row, ks)) || (rc = dev_put(c, &m->csr_val, vv))) { sp_sparse_free(m); return rc; }
  build(cols, num_cols, rows, ptr, oth, ks, vv);
  if ((rc = dev_put(c, &m->col_ptr, ptr)) || (rc = dev_put(c, &m->csc_row, oth)) || (rc = dev_put(c, &m->csc_val, vv))) { sp_sparse_free(m); return rc; }
  {
    std::vector<uint32_t> er(nnz), ec(nnz);
    for (size_t i = 0; i < nnz; i++) { er[i] = (uint32_t)rows[i]; ec[i] = (uint32_t)cols[i]; }
    std::vector<Fq> ev(v, v + nnz);
    if ((rc = dev_put(c, &m->ent_row, er)) || (rc = dev_put(c, &m->ent_col, ec)) || (rc = dev_put(c, &m->ent_val, ev))) { sp_sparse_free(m); return rc; }
  }
  *out = m;
  return SP_OK;
}
// SNARK::encode (lib.rs:325-336 -> sparse_mlpoly.rs:367-427): the row / column addresses of a matrix's entries as a device index list of
// n >= nnz elements (zero-padded: MultiSparseMatPolynomialAsDense pads every matrix to the batch's num_nz_entries), and its values written
// into dst[dst_off, dst_off + n) — both from the entry-order copies kept at upload, device to device.
int32_t sp_sparse_entry_index(sp_ctx* c, const sp_sparse* m, int which, size_t n, sp_index** out) {
  if (!c || !m || !out || (which != 0 && which != 1) || n == 0 || n < m->nnz) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  sp_index* ix = new (std::nothrow) sp_index();
  if (!ix) return SP_ENOMEM;
  ix->ctx = c; ix->n = n; ix->d = nullptr;
  hipError_t e = hipMalloc((void**)&ix->d, 4 * n);
  if (e == hipSuccess && n > m->nnz) e = hipMemsetAsync(ix->d + m->nnz, 0, 4 * (n - m->nnz), c->stream);
  if (e == hipSuccess && m->nnz) e = hipMemcpyAsync(ix->d, which == 0 ? m->ent_row : m->ent_col, 4 * m->nnz, hipMemcpyDeviceToDevice, c->stream);
  if (e != hipSuccess) { if (ix->d) (void)hipFree(ix->d); delete ix; return e == hipErrorOutOfMemory ? SP_ENOMEM : SP_EHIP; }
  *out = ix;
  return SP_OK;
}
int32_t sp_sparse_entry_values(sp_ctx* c, const sp_sparse* m, sp_table* dst, size_t dst_off, size_t n) {
  if (!c || !m || !dst || n < m->nnz || dst_off + n > dst->cap) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  if (n > m->nnz) HIPCHK(hipMemsetAsync(dst->d + dst_off + m->nnz, 0, 32 * (n - m->nnz), c->stream));
  if (m->nnz) HIPCHK(hipMemcpyAsync(dst->d + dst_off, m->ent_val, 32 * m->nnz, hipMemcpyDeviceToDevice, c->stream));
  return SP_OK;
}
void sp_sparse_free(sp_sparse* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->dev);
  (void)hipStreamSynchronize(m->ctx->stream);
  void* ps[] = {m->row_ptr, m->csr_col, m->csr_row, m->csr_val, m->col_ptr, m->csc_row, m->csc_val, m->ent_row, m->ent_col, m->ent_val,
                m->chk_rows, m->chk_first, m->chk_beg, m->chk_end};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  delete m;
}
int32_t sp_sparse_mulvec(sp_ctx* c, const sp_sparse* m, const sp_table* z, sp_table** out) {
  if (!c || !m || !z || !out || z->len < m->num_cols) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  SPCHK(table_new(c, m->num_rows, false, out));
  {
    ProfScope ps(c, PF_SPARSE, (double)m->nnz * (4 + 32 + 32) + 32.0 * (double)m->num_rows);
    hipLaunchKernelGGL(k_spmv, dim3((unsigned)((m->num_rows + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t*)m->row_ptr,
                       (const uint32_t*)m->csr_col, (const Fq*)m->csr_val, (const Fq*)z->d, m->num_rows, (*out)->d);
  }
  return hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;
}
int32_t sp_r1cs_check(sp_ctx* c, const sp_sparse* A, const sp_sparse* B, const sp_sparse* C, const sp_table* z, uint64_t* violated, uint64_t* first_row,
                      uint64_t* rows_out, size_t rows_cap) {
  if (!c || !A || !B || !C || !z || !violated || !first_row) return SP_EINVAL;
  const sp_sparse* ms[3] = {A, B, C};
  const size_t nr = A->num_rows;
  if (B->num_rows != nr || C->num_rows != nr || B->num_cols != A->num_cols || C->num_cols != A->num_cols || z->len < A->num_cols || c->pend_eval.active)
    return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  Csr3 M;
  memset(&M, 0, sizeof M);
  uint32_t total = 0, most = 0;
  double bytes = 4.0 * 3 * (double)(nr + 1);
  for (int k = 0; k < 3; k++) {
    SPCHK(check_plan(c, ms[k]));
    M.row_ptr[k] = ms[k]->row_ptr; M.col[k] = ms[k]->csr_col; M.val[k] = ms[k]->csr_val;
    M.long_rows[k] = ms[k]->chk_rows; M.long_first[k] = ms[k]->chk_first; M.chunk_beg[k] = ms[k]->chk_beg; M.chunk_end[k] = ms[k]->chk_end;
    M.n_long[k] = ms[k]->chk_nrows; M.n_chunks[k] = ms[k]->chk_nchunks; M.part_off[k] = total;
    total += ms[k]->chk_nchunks;
    most = std::max(most, ms[k]->chk_nchunks);
    bytes += (double)ms[k]->nnz * (4 + 32 + 32);
  }
  // scratch: [0, 16) count and first row, [64, ..) the bitmap, then the chunk sums
  const size_t nwords = (nr + 63) / 64, off_part = (64 + 8 * nwords + 31) & ~(size_t)31;
  SPCHK(ensure(&c->scratch, &c->scratch_cap, off_part + 32 * (size_t)total));
  unsigned long long* res = (unsigned long long*)c->scratch;
  unsigned long long* bitmap = (unsigned long long*)((uint8_t*)c->scratch + 64);
  Fq* partials = (Fq*)((uint8_t*)c->scratch + off_part);
  HIPCHK(hipMemsetAsync(res, 0, 8, c->stream));
  HIPCHK(hipMemsetAsync(res + 1, 0xff, 8, c->stream));
  {
    ProfScope ps(c, PF_SPARSE, bytes);
    if (total)
      hipLaunchKernelGGL(k_r1cs_chunks, dim3((most + 3) / 4, 3), dim3(256), 0, c->stream, M, (const Fq*)z->d, partials);
    hipLaunchKernelGGL(k_r1cs_check, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c->stream, M, (const Fq*)z->d, (const Fq*)partials, nr, res, bitmap);
  }
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  uint64_t out[2];
  SPCHK(fetch_out(c, res, out, sizeof out));
  *violated = out[0]; *first_row = out[1];
  if (rows_out && rows_cap && out[0]) {  // the lowest failing indices, from the bitmap
    std::vector<uint64_t> bm(nwords);
    SPCHK(fetch_out(c, bitmap, bm.data(), 8 * nwords));
    size_t n = 0;
    for (size_t w = 0; w < nwords && n < rows_cap; w++)
      for (uint64_t bits = bm[w]; bits && n < rows_cap; bits &= bits - 1) rows_out[n++] = 64 * w + (uint64_t)__builtin_ctzll(bits);
  }
  return SP_OK;
}
int32_t sp_sparse_eval_table(sp_ctx* c, const sp_sparse* const* ms, const uint64_t* w, size_t nm, const sp_table* rx, sp_table** out) {
  if (!c || !ms || !w || !rx || !out || nm == 0 || nm > 3) return SP_EINVAL;
  Csc3 M;
  memset(&M, 0, sizeof M);
  M.nm = (int)nm;
  double bytes = 0;
  for (size_t k = 0; k < nm; k++) {
    if (!ms[k] || ms[k]->num_cols != ms[0]->num_cols || rx->len < ms[k]->num_rows) return SP_EINVAL;
    M.col_ptr[k] = ms[k]->col_ptr; M.row[k] = ms[k]->csc_row; M.val[k] = ms[k]->csc_val;
    memcpy(M.w[k].l, w + 4 * k, 32);
    bytes += (double)ms[k]->nnz * (4 + 32 + 32);
  }
  HIPCHK(hipSetDevice(c->dev));
  size_t nc = ms[0]->num_cols;
  SPCHK(table_new(c, nc, false, out));
  {
    ProfScope ps(c, PF_SPARSE, bytes + 32.0 * (double)nc);
    hipLaunchKernelGGL(k_eval_table, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, c->stream, M, (const Fq*)rx->d, nc, (*out)->d);
  }
  return hipGetLastError() == hipSuccess ? SP_OK : SP_EHIP;
}
int32_t sp_sparse_evaluate(sp_ctx* c, const sp_sparse* m, const sp_table* tx, const sp_table* ty, uint64_t out[4]) {
  if (!c || !m || !tx || !ty || !out || tx->len < m->num_rows || ty->len < m->num_cols) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  size_t nblk = grid_for(m->nnz ? m->nnz : 1, 1024);
  SPCHK(ensure(&c->scratch, &c->scratch_cap, 32 * (nblk + 1)));
  Fq* partials = partials_dst(c, nblk, 1);
  {
    ProfScope ps(c, PF_SPARSE, (double)m->nnz * (8 + 96));
    hipLaunchKernelGGL(k_sparse_eval, dim3((unsigned)nblk), dim3(256), 0, c->stream, (const uint32_t*)m->csr_row, (const uint32_t*)m->csr_col,
                       (const Fq*)m->csr_val, m->nnz, (const Fq*)tx->d, (const Fq*)ty->d, partials);
  }
  return reduce_and_fetch(c, partials, nblk, 1, out);
}

// R1CSInstance::evaluate (r1cs.rs:300-303) of up to four matrices, queued on a low-priority stream of its own and collected with
// sp_job_wait (32 bytes per matrix): SNARK::prove starts it as soon as the second sum-check has fixed ry, and the kernels fill the
// idle time of the witness opening (an inner-product argument: launch-sized kernels and host trips) instead of standing on the
// critical path behind it. tx, ty must stay alive until the job has been waited for.
int32_t sp_sparse_evaluate_begin(sp_ctx* c, const sp_sparse* const* ms, size_t count, const sp_table* tx, const sp_table* ty, sp_job** out) {
  if (!c || !ms || !tx || !ty || !out || count == 0 || count > 4) return SP_EINVAL;
  SparseMany M;
  memset(&M, 0, sizeof M);
  size_t max_nnz = 1;
  double bytes = 0;
  for (size_t k = 0; k < count; k++) {
    if (!ms[k] || tx->len < ms[k]->num_rows || ty->len < ms[k]->num_cols) return SP_EINVAL;
    M.row[k] = ms[k]->csr_row; M.col[k] = ms[k]->csr_col; M.val[k] = ms[k]->csr_val; M.nnz[k] = ms[k]->nnz;
    if (ms[k]->nnz > max_nnz) max_nnz = ms[k]->nnz;
    bytes += (double)ms[k]->nnz * (8 + 96);
  }
  HIPCHK(hipSetDevice(c->dev));
  if (!c->stream_low) return SP_EHIP;
  const size_t nblk = grid_for(max_nnz, 1024);
  sp_job* j = new (std::nothrow) sp_job();
  if (!j) return SP_ENOMEM;
  j->ctx = c; j->rows = count; j->stream = c->stream_low; j->scratch = nullptr;
  j->out_off = 32 * nblk * count;
  j->scratch_bytes = j->out_off + 32 * count;
  int32_t rc = pool_alloc(c, j->scratch_bytes, (void**)&j->scratch);
  if (rc != SP_OK) { delete j; return rc; }
  hipEvent_t ready;
  if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&j->done, hipEventDisableTiming) != hipSuccess) {
    pool_release(c, j->scratch, j->scratch_bytes); delete j; return SP_EHIP;
  }
  (void)hipEventRecord(ready, c->stream);  // tx, ty as produced by what is queued on the main stream
  (void)hipStreamWaitEvent(c->stream_low, ready, 0);
  {
    ProfScope ps(c, PF_SPARSE, bytes, c->stream_low);
    hipLaunchKernelGGL(k_sparse_eval_many, dim3((unsigned)nblk, (unsigned)count), dim3(256), 0, c->stream_low, M, (const Fq*)tx->d, (const Fq*)ty->d, (Fq*)j->scratch);
    hipLaunchKernelGGL(k_sparse_sums, dim3((unsigned)count), dim3(256), 0, c->stream_low, (const Fq*)j->scratch, nblk, (Fq*)(j->scratch + j->out_off));
  }
  (void)hipEventRecord(j->done, c->stream_low);
  (void)hipEventDestroy(ready);
  if (hipGetLastError() != hipSuccess) { (void)hipEventDestroy(j->done); pool_release(c, j->scratch, j->scratch_bytes); delete j; return SP_EHIP; }
  *out = j;
  return SP_OK;
}

}  // extern "C"
