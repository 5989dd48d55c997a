// spartan_amd: device tables of F_q elements (sp_table).
#include "internal.hpp"

extern "C" {
int32_t table_new(sp_ctx* c, size_t len, bool zero, sp_table** out) {
  if (!c || !out || len == 0) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  sp_table* t = new (std::nothrow) sp_table();
  if (!t) return SP_ENOMEM;
  t->ctx = c;
  t->cap = t->len = len;
  t->owner = 1;
  t->d = nullptr;
  t->d_bytes = 32 * len;
  t->alt = nullptr;
  t->alt_bytes = 0;
  int32_t rc = pool_alloc(c, 32 * len, (void**)&t->d);
  if (rc != SP_OK) { delete t; return rc; }
  if (zero && hipMemsetAsync(t->d, 0, 32 * len, c->stream) != hipSuccess) { pool_release(c, t->d, 32 * len); delete t; return SP_EHIP; }
  *out = t;
  return SP_OK;
}
int32_t sp_table_alloc(sp_ctx* c, size_t len, sp_table** out) { return table_new(c, len, true, out); }
int32_t sp_table_alloc_uninit(sp_ctx* c, size_t len, sp_table** out) { return table_new(c, len, false, out); }
int32_t sp_table_write(sp_ctx* c, sp_table* t, size_t off, const uint64_t* Z, size_t len) {
  if (!c || !t || !Z || off + len > t->cap) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipMemcpyAsync(t->d + off, Z, 32 * len, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // caller may reuse Z immediately
  return SP_OK;
}
int32_t sp_table_upload(sp_ctx* c, const uint64_t* Z, size_t len, sp_table** out) {
  if (!Z) return SP_EINVAL;
  SPCHK(table_new(c, len, false, out));
  int32_t rc = sp_table_write(c, *out, 0, Z, len);
  if (rc != SP_OK) { sp_table_free(*out); *out = nullptr; }
  return rc;
}
__global__ void k_copy_small(const Fq* __restrict__ src, size_t n, Fq* __restrict__ dst) { SP_FG_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st_fq(dst + i, ld_fq(src + i));
}
int32_t sp_table_download(sp_ctx* c, const sp_table* t, size_t off, size_t len, uint64_t* out) {
  if (!c || !t || !out || off + len > t->cap) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  if (32 * len <= 4096) {  // a few elements (product-circuit roots, final claims): kernel write into the mapped page + poll
    hipLaunchKernelGGL(k_copy_small, dim3((unsigned)((len + 63) / 64)), dim3(64), 0, c->stream, (const Fq*)(t->d + off), len, (Fq*)hres(c));
    return fetch_small(c, out, 32 * len);
  }
  HIPCHK(hipMemcpyAsync(out, t->d + off, 32 * len, hipMemcpyDeviceToHost, c->stream));
  SPCHK(sync_spin(c));
  return SP_OK;
}
int32_t sp_table_clone(sp_ctx* c, const sp_table* t, sp_table** out) {
  if (!t) return SP_EINVAL;
  SPCHK(table_new(c, t->cap, false, out));
  (*out)->len = t->len;
  HIPCHK(hipMemcpyAsync((*out)->d, t->d, 32 * t->cap, hipMemcpyDeviceToDevice, c->stream));
  return SP_OK;
}
int32_t sp_table_copy(sp_ctx* c, sp_table* dst, size_t dst_off, const sp_table* src, size_t src_off, size_t len) {
  if (!c || !dst || !src || dst_off + len > dst->cap || src_off + len > src->cap) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipMemcpyAsync(dst->d + dst_off, src->d + src_off, 32 * len, hipMemcpyDeviceToDevice, c->stream));
  return SP_OK;
}
size_t sp_table_len(const sp_table* t) { return t ? t->len : 0; }
}  // extern "C"
int32_t table_ensure_alt(sp_table* t, size_t elems) {
  if (t->alt && t->alt_bytes >= 32 * elems) return SP_OK;
  if (t->alt) pool_release(t->ctx, t->alt, t->alt_bytes);
  t->alt = nullptr;
  t->alt_bytes = 0;
  SPCHK(pool_alloc(t->ctx, 32 * elems, (void**)&t->alt));
  t->alt_bytes = 32 * elems;
  return SP_OK;
}
void table_swap_to_alt(sp_table* t, size_t new_len) {
  Fq* old = t->d;
  int old_owned = t->owner;
  size_t old_bytes = t->d_bytes;
  t->d = t->alt; t->owner = 1; t->d_bytes = t->alt_bytes;
  t->cap = t->alt_bytes / 32; t->len = new_len;
  if (old_owned) { t->alt = old; t->alt_bytes = old_bytes; }
  else { t->alt = nullptr; t->alt_bytes = 0; }  // a view's original storage belongs to its parent
}
extern "C" {
void sp_table_free(sp_table* t) {
  if (!t) return;
  (void)hipSetDevice(t->ctx->dev);
  if (t->owner) pool_release(t->ctx, t->d, t->d_bytes);
  if (t->alt) pool_release(t->ctx, t->alt, t->alt_bytes);
  delete t;
}
}  // extern "C"
