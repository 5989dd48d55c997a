// spartan_amd: Instance::new (src/lib.rs:121-227) for one matrix on the device. The caller's entry list — rows[nnz] and cols[nnz] as usize,
// vals[nnz] as canonical 32-byte scalars — becomes a resident sp_sparse (sparse.hip) in three passes, none of them on the host:
//   parse   one lane per entry, in the reference's order (lib.rs:164-186): the index in 64 bits, then the scalar against q; a good entry gets
//           its u32 row, its shifted u32 column and its Montgomery value. The value bytes were copied into ent_val first (a DMA settles their
//           alignment) and are converted there in place, as assign.hip converts an assignment.
//   CSR     a stable radix sort of (row, position) with rocPRIM, the row pointers as the lower bound of every row number in the sorted keys,
//           one gather of (column, value) through the sorted positions
//   CSC     the same by column
// Within a row (column) the order is entry order, as sp_sparse_upload's stable counting sort leaves it: both builds give the same arrays.
#include <rocprim/device/device_radix_sort.hpp>

#include "internal.hpp"

constexpr unsigned BUILD_BLOCK = 256;  // threads of a workgroup; every grid here is ceil(n / BUILD_BLOCK) workgroups, never capped: one lane per element

// A wavefront owns 64 consecutive entries, a lane one of them. Entries [nnz, total) are the reference's explicit zero constraints
// (lib.rs:191-195): (row = e, col = pad_col, val = 0). res[0] += entries with a bad index, res[1] = min(res[1], the lowest of them),
// res[2] += entries with a good index and a value >= q, res[3] = min(res[3], the lowest of them): at most two atomicAdd and two atomicMin
// per wavefront (the pattern of k_assign_check and k_r1cs_check), so the report does not depend on the launch geometry. An entry that
// fails either test writes nothing; the caller drops the matrix.
__global__ void __launch_bounds__(BUILD_BLOCK) k_build_parse(const uint64_t* __restrict__ rows, const uint64_t* __restrict__ cols, Fq* __restrict__ val,
                                                             size_t nnz, size_t total, uint64_t row_limit, uint64_t col_limit, uint64_t col_split,
                                                             uint64_t col_shift, uint32_t pad_col, uint32_t* __restrict__ ent_row,
                                                             uint32_t* __restrict__ ent_col, unsigned long long* __restrict__ res) {
  const unsigned lane = threadIdx.x & 63;
  const size_t e = (size_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
  const size_t base = e - lane;  // first entry of the wavefront
  if (base >= total) return;     // the whole wavefront
  bool bad_index = false, bad_scalar = false;
  if (e < nnz) {
    const uint64_t r = rows[e], c = cols[e];  // compared as 64-bit values: 2^32 + r is a bad index, not row r
    bad_index = r >= row_limit || c >= col_limit;
    if (!bad_index) {
      const Fq x = ld_fq(val + e);
      bad_scalar = !fq_is_canonical(x);
      if (!bad_scalar) {
        ent_row[e] = (uint32_t)r;
        ent_col[e] = (uint32_t)(c >= col_split ? c + col_shift : c);  // lib.rs:178-182
        st_fq(val + e, fq_to_mont(x));
      }
    }
  } else if (e < total) {
    ent_row[e] = (uint32_t)e;
    ent_col[e] = pad_col;
    st_fq(val + e, fq_zero());
  }
  const unsigned long long mi = __ballot(bad_index), ms = __ballot(bad_scalar);
  if (lane == 0 && mi) {
    atomicAdd(res, (unsigned long long)__popcll(mi));
    atomicMin(res + 1, (unsigned long long)(base + (size_t)(__ffsll(mi) - 1)));
  }
  if (lane == 0 && ms) {
    atomicAdd(res + 2, (unsigned long long)__popcll(ms));
    atomicMin(res + 3, (unsigned long long)(base + (size_t)(__ffsll(ms) - 1)));
  }
}
__global__ void __launch_bounds__(BUILD_BLOCK) k_build_iota(uint32_t* __restrict__ pos, size_t n) {
  const size_t i = (size_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
  if (i < n) pos[i] = (uint32_t)i;
}
// ptr[k] = the number of entries with a key below k = where the run of key k begins in the sorted keys, for k in [0, nkeys]: a lower bound
// per key, at most 32 steps whatever the distribution (no atomics on one counter when every entry shares a row, no lane that walks a gap)
__global__ void __launch_bounds__(BUILD_BLOCK) k_build_ptr(const uint32_t* __restrict__ sorted, uint32_t n, size_t nkeys, uint32_t* __restrict__ ptr) {
  const size_t k = (size_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
  if (k > nkeys) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((size_t)sorted[mid] < k) lo = mid + 1; else hi = mid;
  }
  ptr[k] = lo;
}
// the sorted copy through the sorted positions: one 32-byte element per lane (two 16-byte accesses each way) and its other coordinate
__global__ void __launch_bounds__(BUILD_BLOCK) k_build_gather(const uint32_t* __restrict__ pos, size_t n, const uint32_t* __restrict__ ent_other,
                                                              const Fq* __restrict__ ent_val, uint32_t* __restrict__ other, Fq* __restrict__ val) {
  const size_t q = (size_t)blockIdx.x * BUILD_BLOCK + threadIdx.x;
  if (q >= n) return;
  const uint32_t p = pos[q];
  other[q] = ent_other[p];
  st_fq(val + q, ld_fq(ent_val + p));
}

static inline dim3 build_grid(size_t n) { return dim3((unsigned)((n + BUILD_BLOCK - 1) / BUILD_BLOCK)); }
static inline unsigned key_bits(size_t nkeys) {  // the bits a key below nkeys can have set, at least 1
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < nkeys) bits++;
  return bits;
}
template <typename T>
static int32_t dev_array(T** d, size_t n) {
  HIPCHK(hipMalloc((void**)d, sizeof(T) * (n ? n : 1)));
  return SP_OK;
}

static int32_t sparse_from_entries(sp_ctx* c, const uint64_t* rows, const uint64_t* cols, const uint8_t* vals, hipMemcpyKind kind, size_t nnz,
                                   uint64_t row_limit, uint64_t col_limit, uint64_t col_split, uint64_t col_shift, size_t pad_count, uint64_t pad_col,
                                   size_t num_rows, size_t num_cols, sp_sparse** out, uint64_t* report) {
  if (!c || !out || (nnz && (!rows || !cols || !vals)) || num_rows == 0 || num_cols == 0 || num_rows > 0xffffffffULL || num_cols > 0xffffffffULL)
    return SP_EINVAL;
  if (nnz >= 0xffffffffULL || pad_count >= 0xffffffffULL || nnz + pad_count >= 0xffffffffULL) return SP_EINVAL;
  if (row_limit > num_rows || col_shift > num_cols || col_limit > num_cols - col_shift) return SP_EINVAL;
  if (pad_count && (nnz + pad_count > num_rows || pad_col >= num_cols)) return SP_EINVAL;  // a pad entry is (its own number, pad_col)
  const size_t total = nnz + pad_count;
  HIPCHK(hipSetDevice(c->dev));
  const unsigned row_bits = key_bits(num_rows), col_bits = key_bits(num_cols);
  size_t tmp_r = 0, tmp_c = 0;
  if (total) {
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_r, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, total, 0u,
                                     row_bits, c->stream));
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_c, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, total, 0u,
                                     col_bits, c->stream));
  }
  const size_t tmp = tmp_r > tmp_c ? tmp_r : tmp_c;
  const size_t a8 = (8 * nnz + 255) & ~(size_t)255, a4 = (4 * total + 255) & ~(size_t)255;
  // scratch2: [report][rows][cols][sorted keys][positions][sorted positions][library temp]
  HIPCHK(hipStreamSynchronize(c->stream));
  SPCHK(ensure(&c->scratch2, &c->scratch2_cap, 256 + 2 * a8 + 3 * a4 + tmp + 256));
  uint8_t* base = (uint8_t*)c->scratch2;
  unsigned long long* res = (unsigned long long*)base;
  uint64_t *drows = (uint64_t*)(base + 256), *dcols = (uint64_t*)(base + 256 + a8);
  uint32_t *kout = (uint32_t*)(base + 256 + 2 * a8), *pin = (uint32_t*)(base + 256 + 2 * a8 + a4), *pout = (uint32_t*)(base + 256 + 2 * a8 + 2 * a4);
  void* lib = base + 256 + 2 * a8 + 3 * a4;

  sp_sparse* m = new (std::nothrow) sp_sparse();
  if (!m) return SP_ENOMEM;
  memset(m, 0, sizeof *m);
  m->ctx = c; m->nnz = total; m->num_rows = num_rows; m->num_cols = num_cols;
  uint64_t rep[4] = {0, UINT64_MAX, 0, UINT64_MAX};
  auto run = [&]() -> int32_t {
    SPCHK(dev_array(&m->ent_row, total)); SPCHK(dev_array(&m->ent_col, total)); SPCHK(dev_array(&m->ent_val, total));
    SPCHK(dev_array(&m->row_ptr, num_rows + 1)); SPCHK(dev_array(&m->csr_col, total)); SPCHK(dev_array(&m->csr_row, total)); SPCHK(dev_array(&m->csr_val, total));
    SPCHK(dev_array(&m->col_ptr, num_cols + 1)); SPCHK(dev_array(&m->csc_row, total)); SPCHK(dev_array(&m->csc_val, total));
    if (total == 0) {  // an empty matrix: pointers only
      HIPCHK(hipMemsetAsync(m->row_ptr, 0, 4 * (num_rows + 1), c->stream));
      HIPCHK(hipMemsetAsync(m->col_ptr, 0, 4 * (num_cols + 1), c->stream));
      return SP_OK;
    }
    if (nnz) {
      HIPCHK(hipMemcpyAsync(drows, rows, 8 * nnz, kind, c->stream));
      HIPCHK(hipMemcpyAsync(dcols, cols, 8 * nnz, kind, c->stream));
      HIPCHK(hipMemcpyAsync(m->ent_val, vals, 32 * nnz, kind, c->stream));
    }
    HIPCHK(hipMemsetAsync(res, 0xff, 32, c->stream));
    HIPCHK(hipMemsetAsync(res, 0, 8, c->stream));
    HIPCHK(hipMemsetAsync(res + 2, 0, 8, c->stream));
    {
      ProfScope ps(c, PF_SPARSE, (16.0 + 64.0 + 8.0) * (double)nnz);
      hipLaunchKernelGGL(k_build_parse, build_grid(total), dim3(BUILD_BLOCK), 0, c->stream, (const uint64_t*)drows, (const uint64_t*)dcols, m->ent_val, nnz,
                         total, row_limit, col_limit, col_split, col_shift, (uint32_t)pad_col, m->ent_row, m->ent_col, res);
    }
    if (hipGetLastError() != hipSuccess) return SP_EHIP;
    SPCHK(fetch_out(c, res, rep, sizeof rep));  // waits: the caller may reuse its arrays when this returns
    if (rep[0] || rep[2]) return rep[1] < rep[3] ? SP_EINDEX : SP_ESCALAR;  // the lowest failing entry decides, as the reference's loop does
    {
      ProfScope ps(c, PF_SPARSE, 2.0 * (double)total * (4 * 10 + 4 + 4 + 64) + 4.0 * (double)(num_rows + num_cols));
      hipLaunchKernelGGL(k_build_iota, build_grid(total), dim3(BUILD_BLOCK), 0, c->stream, pin, total);
      HIPCHK(rocprim::radix_sort_pairs(lib, tmp_r, (const uint32_t*)m->ent_row, m->csr_row, (const uint32_t*)pin, pout, total, 0u, row_bits, c->stream));
      hipLaunchKernelGGL(k_build_ptr, build_grid(num_rows + 1), dim3(BUILD_BLOCK), 0, c->stream, (const uint32_t*)m->csr_row, (uint32_t)total, num_rows, m->row_ptr);
      hipLaunchKernelGGL(k_build_gather, build_grid(total), dim3(BUILD_BLOCK), 0, c->stream, (const uint32_t*)pout, total, (const uint32_t*)m->ent_col,
                         (const Fq*)m->ent_val, m->csr_col, m->csr_val);
      HIPCHK(rocprim::radix_sort_pairs(lib, tmp_c, (const uint32_t*)m->ent_col, kout, (const uint32_t*)pin, pout, total, 0u, col_bits, c->stream));
      hipLaunchKernelGGL(k_build_ptr, build_grid(num_cols + 1), dim3(BUILD_BLOCK), 0, c->stream, (const uint32_t*)kout, (uint32_t)total, num_cols, m->col_ptr);
      hipLaunchKernelGGL(k_build_gather, build_grid(total), dim3(BUILD_BLOCK), 0, c->stream, (const uint32_t*)pout, total, (const uint32_t*)m->ent_row,
                         (const Fq*)m->ent_val, m->csc_row, m->csc_val);
    }
    if (hipGetLastError() != hipSuccess) return SP_EHIP;
    return SP_OK;
  };
  int32_t rc = run();
  if (hipStreamSynchronize(c->stream) != hipSuccess && rc == SP_OK) rc = SP_EHIP;  // scratch2 is shared with other calls
  if ((rc == SP_OK || rc == SP_EINDEX || rc == SP_ESCALAR) && report) memcpy(report, rep, sizeof rep);
  if (rc != SP_OK) { sp_sparse_free(m); m = nullptr; }
  *out = m;
  return rc;
}

extern "C" {
int32_t sp_sparse_from_entries(sp_ctx* c, const uint64_t* rows, const uint64_t* cols, const uint8_t* vals, size_t nnz, uint64_t row_limit, uint64_t col_limit,
                               uint64_t col_split, uint64_t col_shift, size_t pad_count, uint64_t pad_col, size_t num_rows, size_t num_cols, sp_sparse** out,
                               uint64_t* report) {
  return sparse_from_entries(c, rows, cols, vals, hipMemcpyHostToDevice, nnz, row_limit, col_limit, col_split, col_shift, pad_count, pad_col, num_rows,
                             num_cols, out, report);
}
int32_t sp_sparse_from_entries_dev(sp_ctx* c, const uint64_t* dev_rows, const uint64_t* dev_cols, const uint8_t* dev_vals, size_t nnz, uint64_t row_limit,
                                   uint64_t col_limit, uint64_t col_split, uint64_t col_shift, size_t pad_count, uint64_t pad_col, size_t num_rows,
                                   size_t num_cols, sp_sparse** out, uint64_t* report) {
  return sparse_from_entries(c, dev_rows, dev_cols, dev_vals, hipMemcpyDeviceToDevice, nnz, row_limit, col_limit, col_split, col_shift, pad_count, pad_col,
                             num_rows, num_cols, out, report);
}
int32_t sp_sparse_download_entries(sp_ctx* c, const sp_sparse* m, uint32_t* rows, uint32_t* cols, uint64_t* vals) {
  if (!c || !m || (m->nnz && (!rows || !cols || !vals))) return SP_EINVAL;
  if (m->nnz == 0) return SP_OK;
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipMemcpyAsync(rows, m->ent_row, 4 * m->nnz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(cols, m->ent_col, 4 * m->nnz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(vals, m->ent_val, 32 * m->nnz, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return SP_OK;
}
}  // extern "C"
