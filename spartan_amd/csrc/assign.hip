// spartan_amd: canonical scalar bytes <-> device tables (Assignment::new, src/lib.rs:62-88; Scalar::from_bytes / to_bytes,
// ristretto255.rs:390-431). The bytes are copied into the table's own allocation first (a DMA settles their alignment; on a little-endian
// host the 32 bytes of a scalar ARE its four limbs), then one lane per scalar reads its whole element, compares it with q and, when it is
// below q, writes its Montgomery form back over it. A lane owns 32 contiguous bytes: the layout of every F_q table here (two 16-byte
// accesses per lane, a wavefront covers 2 KiB without a gap). One read and one write of the table in HBM, nothing else.
#include "internal.hpp"

constexpr unsigned ASSIGN_BLOCK = 256;  // threads of a workgroup; the grid is ceil(n / ASSIGN_BLOCK) workgroups, never capped: one lane per scalar

// A wavefront owns 64 consecutive entries, a lane one of them. CONVERT: an entry below q is replaced by its Montgomery form (an entry >= q
// is left as it came; the caller drops the table). res[0] += entries >= q, res[1] = min(res[1], idx_base + the lowest such index): one
// atomicAdd and one atomicMin per wavefront that found any (the pattern of k_r1cs_check, sparse.hip), so the report does not depend on the
// launch geometry or on the order in which wavefronts retire.
template <bool CONVERT>
__global__ void __launch_bounds__(ASSIGN_BLOCK) k_assign_check(Fq* __restrict__ d, size_t n, size_t idx_base, unsigned long long* __restrict__ res) {
  const unsigned lane = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * ASSIGN_BLOCK + threadIdx.x;
  const size_t base = i - lane;  // first entry of the wavefront
  if (base >= n) return;         // the whole wavefront
  const bool live = i < n;
  Fq x = fq_zero();
  if (live) x = ld_fq(d + i);
  const bool bad = live && !fq_is_canonical(x);
  if (CONVERT && live && !bad) st_fq(d + i, fq_to_mont(x));
  const unsigned long long mask = __ballot(bad);
  if (lane == 0 && mask) {
    atomicAdd(res, (unsigned long long)__popcll(mask));
    atomicMin(res + 1, (unsigned long long)(idx_base + base + (size_t)(__ffsll(mask) - 1)));
  }
}
// Scalar::to_bytes (ristretto255.rs:419-431): dst[i] = the canonical integer of src[i]; its four limbs are the 32 little-endian bytes
__global__ void __launch_bounds__(ASSIGN_BLOCK) k_assign_canonical(const Fq* __restrict__ src, size_t n, Fq* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * ASSIGN_BLOCK + threadIdx.x;
  if (i < n) st_fq(dst + i, fq_from_mont(ld_fq(src + i)));
}

// 32 n bytes fit in device memory, so ceil(n / ASSIGN_BLOCK) is far below the 2^31 - 1 workgroups a grid may have
static inline dim3 assign_grid(size_t n) { return dim3((unsigned)((n + ASSIGN_BLOCK - 1) / ASSIGN_BLOCK)); }

// the comparison (and the conversion) over d[0, n), and the 16-byte device report fetched: one round trip
static int32_t assign_check(sp_ctx* c, Fq* d, size_t n, size_t idx_base, bool convert, uint64_t rep[2]) {
  unsigned long long* res = nullptr;
  SPCHK(pool_alloc(c, 16, (void**)&res));
  auto run = [&]() -> int32_t {
    HIPCHK(hipMemsetAsync(res, 0, 8, c->stream));
    HIPCHK(hipMemsetAsync(res + 1, 0xff, 8, c->stream));
    {
      ProfScope ps(c, PF_MISC, (convert ? 64.0 : 32.0) * (double)n);
      if (convert) hipLaunchKernelGGL(k_assign_check<true>, assign_grid(n), dim3(ASSIGN_BLOCK), 0, c->stream, d, n, idx_base, res);
      else hipLaunchKernelGGL(k_assign_check<false>, assign_grid(n), dim3(ASSIGN_BLOCK), 0, c->stream, d, n, idx_base, res);
    }
    if (hipGetLastError() != hipSuccess) return SP_EHIP;
    return fetch_out(c, res, rep, 16);
  };
  const int32_t rc = run();
  pool_release(c, res, 16);
  return rc;
}
static bool range_ok(const sp_ctx* c, const sp_table* t, size_t off, size_t len) {
  return len != 0 && off <= t->len && len <= t->len - off && t->ctx->dev == c->dev;
}
static int32_t table_from_bytes(sp_ctx* c, const uint8_t* bytes, hipMemcpyKind kind, size_t n, sp_table** out, uint64_t* report) {
  if (!c || !bytes || !out || n == 0) return SP_EINVAL;
  sp_table* t = nullptr;
  SPCHK(table_new(c, n, false, &t));  // sets the device
  uint64_t rep[2] = {0, UINT64_MAX};
  int32_t rc = SP_OK;
  if (hipMemcpyAsync(t->d, bytes, 32 * n, kind, c->stream) != hipSuccess) rc = SP_EHIP;
  if (rc == SP_OK) rc = assign_check(c, t->d, n, 0, true, rep);  // waits: the caller may reuse `bytes` when this returns
  if (rc == SP_OK && rep[0]) rc = SP_ESCALAR;
  if (rc == SP_OK || rc == SP_ESCALAR) {
    if (report) { report[0] = rep[0]; report[1] = rep[1]; }
  }
  if (rc != SP_OK) { sp_table_free(t); t = nullptr; }
  *out = t;
  return rc;
}

extern "C" {
int32_t sp_table_from_bytes(sp_ctx* c, const uint8_t* bytes, size_t n, sp_table** out, uint64_t* report) {
  return table_from_bytes(c, bytes, hipMemcpyHostToDevice, n, out, report);
}
int32_t sp_table_from_bytes_dev(sp_ctx* c, const uint8_t* dev_bytes, size_t n, sp_table** out, uint64_t* report) {
  return table_from_bytes(c, dev_bytes, hipMemcpyDeviceToDevice, n, out, report);
}
int32_t sp_table_to_bytes(sp_ctx* c, const sp_table* t, size_t off, size_t len, uint8_t* out) {
  if (!c || !t || !out || !range_ok(c, t, off, len)) return SP_EINVAL;
  sp_table* s = nullptr;
  SPCHK(table_new(c, len, false, &s));
  {
    ProfScope ps(c, PF_MISC, 64.0 * (double)len);
    hipLaunchKernelGGL(k_assign_canonical, assign_grid(len), dim3(ASSIGN_BLOCK), 0, c->stream, (const Fq*)(t->d + off), len, s->d);
  }
  int32_t rc = hipGetLastError() != hipSuccess ? SP_EHIP : SP_OK;
  if (rc == SP_OK && hipMemcpyAsync(out, s->d, 32 * len, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = SP_EHIP;
  if (rc == SP_OK) rc = sync_spin(c);
  sp_table_free(s);  // back to the pool, which is stream-ordered
  return rc;
}
int32_t sp_table_check_reduced(sp_ctx* c, const sp_table* t, size_t off, size_t len, uint64_t* report) {
  if (!c || !t || !range_ok(c, t, off, len)) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  uint64_t rep[2] = {0, UINT64_MAX};
  SPCHK(assign_check(c, t->d + off, len, off, false, rep));
  if (report) { report[0] = rep[0]; report[1] = rep[1]; }
  return SP_OK;
}
}  // extern "C"
