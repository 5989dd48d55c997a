// spartan_amd: the device's share of R1CSShape::get_digest (src/r1cs.rs:154-158). The digest is the zlib stream of bincode(shape) as miniz's
// tdefl writes it at level 6 (spartan_amd/host/deflate.cc restates tdefl). Two things run here:
//   sp_sparse_bincode    the matrices' part of bincode(R1CSShape), serialised from the resident entries into a device byte buffer
//   sp_deflate_*         tdefl's hash-chain match search, one input position per lane
// The parser that consumes the matches, the block decisions and the Huffman coding are sequential and stay on the host.
//
// The search, per position p of the input D[0, n) (names as in deflate.cc, find_match):
//   links   h(p) = ((D[p] << 10) ^ (D[p+1] << 5) ^ D[p+2]) & 32767;  L[p] = low 16 bits of the greatest q < p with h(q) == h(p), else 0.
//           Within a segment: a stable radix sort of the positions by h (rocPRIM); an element takes the position before it in its group,
//           the first of a group takes the head carried from the segments before; the last of a group becomes the new head.
//   find    find_match with lookahead min(258, n - p), dict_size min(p, 32768 - lookahead), dict[q + k] = D[q + k] and next[q] = L[q]:
//           within dict_size the ring slots tdefl reads still hold exactly these. Probe budget, three-hop inner loop, c0/c1 filter, the
//           dist == 0 break and the early return at the longest match are as in the host code.
//   A[p] = find(p, 2);  B[p] = find(p, len(A[p-1])) where A[p-1] leaves the parser's filter as a held match.
// A segment needs of its predecessors: head[32768], the last 32768 links, A[first - 1]. Every index below is bounded by construction:
//   D[p + k], k < lookahead <= n - p;  D[cand + k], cand < p;  L window index cand - first + 32768 with cand >= p - 32768 + lookahead >= first - 32768.
#include <rocprim/device/device_radix_sort.hpp>

#include "internal.hpp"

namespace {
constexpr unsigned DM_BLOCK = 256;       // one position per lane, four wavefronts a workgroup
constexpr unsigned DM_DICT = 32768, DM_MAXM = 258, DM_MINM = 3, DM_HBITS = 15;
constexpr size_t DM_AHEAD = DM_MAXM;     // bytes past a segment's end its parser reads (the lookahead of its last position)

__device__ __forceinline__ unsigned dm_hash(const uint8_t* __restrict__ D, size_t p) {
  return (((unsigned)D[p] << 10) ^ ((unsigned)D[p + 1] << 5) ^ (unsigned)D[p + 2]) & (DM_DICT - 1);
}
// keys[i] = h(first + i), vals[i] = i for the m positions of the segment that have three bytes
__global__ void __launch_bounds__(DM_BLOCK) k_dm_hash(const uint8_t* __restrict__ D, size_t first, uint32_t m, uint16_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= m) return;
  keys[i] = (uint16_t)dm_hash(D, first + i);
  vals[i] = i;
}
// sorted (stable) by hash: within a group the positions ascend
__global__ void __launch_bounds__(DM_BLOCK) k_dm_links(const uint16_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t m, unsigned first_lo,
                                                       const uint16_t* __restrict__ head, uint16_t* __restrict__ Lseg) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= m) return;
  const uint16_t k = keys[i];
  const bool group_first = i == 0 || keys[i - 1] != k;
  Lseg[vals[i]] = group_first ? head[k] : (uint16_t)(first_lo + vals[i - 1]);
}
// a launch of its own: every read of head[] by k_dm_links is behind us
__global__ void __launch_bounds__(DM_BLOCK) k_dm_heads(const uint16_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t m, unsigned first_lo,
                                                       uint16_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= m) return;
  const uint16_t k = keys[i];
  if (i == m - 1 || keys[i + 1] != k) head[k] = (uint16_t)(first_lo + vals[i]);
}

__device__ __forceinline__ uint32_t dm_pack(unsigned dist, unsigned len) { return dist | (len << 16); }
__device__ __forceinline__ uint32_t dm_ld32(const uint8_t* p) {  // any alignment
  uint32_t x;
  __builtin_memcpy(&x, p, 4);
  return x;
}
// Lw[q - first + 32768] = L[q]
__device__ uint32_t dm_find(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, size_t first, size_t p, unsigned init, unsigned mp0,
                            unsigned mp1) {
  const size_t left = n - p;
  const unsigned la = left < DM_MAXM ? (unsigned)left : DM_MAXM;
  const unsigned max_dist = p < (size_t)(DM_DICT - la) ? (unsigned)p : DM_DICT - la;
  unsigned dist = 0, best = 0, match_len = init;
  if (la <= match_len) return dm_pack(0, init);
  unsigned probes_left = match_len >= 32 ? mp1 : mp0;
  const uint8_t* s = D + p;
  uint8_t c0 = s[match_len], c1 = s[match_len - 1];
  size_t cand = p;
  for (;;) {
    for (;;) {
      if (--probes_left == 0) return dm_pack(best, match_len);
      bool hit = false;
#pragma unroll 1
      for (int k = 0; k < 3 && !hit; k++) {
        const unsigned nx = Lw[(cand + DM_DICT) - first];
        if (!nx || (dist = (((unsigned)p - nx) & 0xFFFFu)) > max_dist) return dm_pack(best, match_len);
        cand = p - dist;
        if (D[cand + match_len] == c0 && D[cand + match_len - 1] == c1) hit = true;
      }
      if (hit) break;
    }
    if (!dist) break;
    const uint8_t* q = D + cand;
    unsigned probe_len = 0;
    bool differ = false;
    while (probe_len + 4 <= la) {
      const uint32_t x = dm_ld32(s + probe_len) ^ dm_ld32(q + probe_len);
      if (x) { probe_len += (unsigned)(__ffs((int)x) - 1) >> 3; differ = true; break; }
      probe_len += 4;
    }
    if (!differ)
      while (probe_len < la && s[probe_len] == q[probe_len]) probe_len++;
    if (probe_len > match_len) {
      best = dist;
      if ((match_len = probe_len) == la) break;
      c0 = s[match_len]; c1 = s[match_len - 1];
    }
  }
  return dm_pack(best, match_len);
}
// does A[pos] = a leave the parser's filter as a held match (deflate.cc, held_after_filter)
__device__ __forceinline__ bool dm_held(uint32_t a, size_t pos) {
  const unsigned dist = a & 0xFFFFu, len = a >> 16;
  if (!dist) return false;
  if ((len == DM_MINM && dist >= 8192u) || (unsigned)(pos & (DM_DICT - 1)) == dist) return false;
  return len < 128;
}
// Ab[0] = A[first - 1] (0 before the first position), Ab[1 + i] = A[first + i]
__global__ void __launch_bounds__(DM_BLOCK) k_dm_search_a(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, size_t first, uint32_t count,
                                                          unsigned mp0, unsigned mp1, uint32_t* __restrict__ Ab) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= count) return;
  Ab[1 + i] = dm_find(D, n, Lw, first, first + i, DM_MINM - 1, mp0, mp1);
}
__global__ void __launch_bounds__(DM_BLOCK) k_dm_search_b(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, size_t first, uint32_t count,
                                                          unsigned mp0, unsigned mp1, const uint32_t* __restrict__ Ab, uint32_t* __restrict__ Bb) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= count) return;
  const size_t p = first + i;
  const uint32_t a = Ab[i];
  Bb[i] = (p && dm_held(a, p - 1)) ? dm_find(D, n, Lw, first, p, a >> 16, mp0, mp1) : 0u;
}

// one 8-byte word per lane: words 0..2 the matrix's header, then six words an entry
__global__ void __launch_bounds__(DM_BLOCK) k_sparse_bincode(const uint32_t* __restrict__ ent_row, const uint32_t* __restrict__ ent_col,
                                                             const uint64_t* __restrict__ ent_val, size_t nnz, uint64_t nvx, uint64_t nvy,
                                                             uint64_t* __restrict__ out) {
  const size_t w = (size_t)blockIdx.x * DM_BLOCK + threadIdx.x;
  if (w >= 3 + 6 * nnz) return;
  uint64_t v;
  if (w < 3) {
    v = w == 0 ? nvx : (w == 1 ? nvy : (uint64_t)nnz);
  } else {
    const size_t e = (w - 3) / 6, f = (w - 3) % 6;
    v = f == 0 ? (uint64_t)ent_row[e] : (f == 1 ? (uint64_t)ent_col[e] : ent_val[4 * e + (f - 2)]);
  }
  out[w] = v;
}
static inline dim3 dm_grid(size_t n) { return dim3((unsigned)((n + DM_BLOCK - 1) / DM_BLOCK)); }
}  // namespace

struct sp_deflate {
  sp_ctx* ctx = nullptr;
  hipStream_t st = nullptr;
  size_t n = 0, seg = 0, nseg = 0, started = 0;
  unsigned mp[2] = {0, 0};
  const uint8_t* dD = nullptr;
  uint8_t* dD_own = nullptr;
  uint16_t *head = nullptr, *Lw = nullptr, *keys_in = nullptr, *keys_out = nullptr;
  uint32_t *Ab = nullptr, *Bb = nullptr, *vals_in = nullptr, *vals_out = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2][5] = {{nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr}};
  size_t first_of(size_t s) const { return s * seg; }
  size_t count_of(size_t s) const { return n - s * seg < seg ? n - s * seg : seg; }
  // pinned slot: [A: 4 seg][B: 4 seg][L: 2 seg][bytes: seg + DM_AHEAD]
  uint32_t* pA(int k) const { return (uint32_t*)pin[k]; }
  uint32_t* pB(int k) const { return (uint32_t*)(pin[k] + 4 * seg); }
  uint16_t* pL(int k) const { return (uint16_t*)(pin[k] + 8 * seg); }
  uint8_t* pD(int k) const { return pin[k] + 10 * seg; }
};

extern "C" {
void sp_deflate_close(sp_deflate* d) {
  if (!d) return;
  (void)hipSetDevice(d->ctx->dev);
  if (d->st) (void)hipStreamSynchronize(d->st);
  for (auto& slot : d->ev)
    for (hipEvent_t e : slot)
      if (e) (void)hipEventDestroy(e);
  for (uint8_t* p : d->pin)
    if (p) (void)hipHostFree(p);
  for (void* p : {(void*)d->dD_own, (void*)d->head, (void*)d->Lw, (void*)d->keys_in, (void*)d->keys_out, (void*)d->Ab, (void*)d->Bb, (void*)d->vals_in,
                  (void*)d->vals_out, d->tmp})
    if (p) (void)hipFree(p);
  if (d->st) (void)hipStreamDestroy(d->st);
  delete d;
}

static int32_t deflate_open(sp_deflate* d, const uint8_t* data, int on_device) {
  sp_ctx* c = d->ctx;
  const size_t seg = d->seg;
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking));
  if (d->nseg == 0) return SP_OK;
  for (auto& slot : d->ev)
    for (hipEvent_t& e : slot) HIPCHK(hipEventCreate(&e));
  if (on_device) {
    d->dD = data;
  } else {
    HIPCHK(hipMalloc((void**)&d->dD_own, d->n));
    HIPCHK(hipMemcpyAsync(d->dD_own, data, d->n, hipMemcpyHostToDevice, d->st));
    d->dD = d->dD_own;
  }
  // the library's temporary storage: the larger of what a full segment and what the last (shorter) one ask for
  const size_t last = d->n - (d->nseg - 1) * seg, last_m = last > 2 ? last - 2 : 1;
  size_t tmp_last = 0;
  HIPCHK(rocprim::radix_sort_pairs(nullptr, d->tmp_bytes, (const uint16_t*)nullptr, (uint16_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, seg, 0u,
                                   DM_HBITS, d->st));
  HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_last, (const uint16_t*)nullptr, (uint16_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, last_m, 0u,
                                   DM_HBITS, d->st));
  if (tmp_last > d->tmp_bytes) d->tmp_bytes = tmp_last;
  HIPCHK(hipMalloc(&d->tmp, d->tmp_bytes ? d->tmp_bytes : 256));
  HIPCHK(hipMalloc((void**)&d->head, 2 * DM_DICT));
  HIPCHK(hipMalloc((void**)&d->Lw, 2 * (DM_DICT + seg)));
  HIPCHK(hipMalloc((void**)&d->keys_in, 2 * seg));
  HIPCHK(hipMalloc((void**)&d->keys_out, 2 * seg));
  HIPCHK(hipMalloc((void**)&d->vals_in, 4 * seg));
  HIPCHK(hipMalloc((void**)&d->vals_out, 4 * seg));
  HIPCHK(hipMalloc((void**)&d->Ab, 4 * (seg + 1)));
  HIPCHK(hipMalloc((void**)&d->Bb, 4 * seg));
  for (uint8_t*& p : d->pin) HIPCHK(hipHostMalloc((void**)&p, 11 * seg + DM_AHEAD, hipHostMallocDefault));
  HIPCHK(hipMemsetAsync(d->head, 0, 2 * DM_DICT, d->st));
  HIPCHK(hipMemsetAsync(d->Lw, 0, 2 * DM_DICT, d->st));
  HIPCHK(hipMemsetAsync(d->Ab, 0, 4, d->st));
  return SP_OK;
}
int32_t sp_deflate_open(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, sp_deflate** out) {
  if (!c || !out || (n && !data) || probes == 0 || probes > 0xFFF) return SP_EINVAL;
  sp_deflate* d = new (std::nothrow) sp_deflate();
  if (!d) return SP_ENOMEM;
  d->ctx = c;
  d->n = n;
  const size_t opt = (size_t)c->opt.v[OPT_DIGEST_SEGMENT];
  d->seg = n < opt ? (n < DM_DICT ? DM_DICT : n) : opt;  // a short input is one segment of its own length (never below the window)
  d->nseg = (n + d->seg - 1) / d->seg;
  d->mp[0] = 1 + (probes + 2) / 3;
  d->mp[1] = 1 + ((probes >> 2) + 2) / 3;
  const int32_t rc = deflate_open(d, data, on_device);
  if (rc != SP_OK) { sp_deflate_close(d); d = nullptr; }
  *out = d;
  return rc;
}
size_t sp_deflate_segments(const sp_deflate* d) { return d ? d->nseg : 0; }

int32_t sp_deflate_segment_start(sp_deflate* d, size_t s) {
  if (!d || s >= d->nseg || s != d->started) return SP_EINVAL;
  sp_ctx* c = d->ctx;
  HIPCHK(hipSetDevice(c->dev));
  const int k = (int)(s & 1);
  const size_t first = d->first_of(s), count = d->count_of(s), n = d->n;
  // positions of the segment that have three bytes: p + 2 < n
  const size_t m = n >= 3 && first < n - 2 ? (first + count <= n - 2 ? count : n - 2 - first) : 0;
  uint16_t* Lseg = d->Lw + DM_DICT;
  hipStream_t st = d->st;
  HIPCHK(hipEventRecord(d->ev[k][0], st));
  if (m < count) HIPCHK(hipMemsetAsync(Lseg + m, 0, 2 * (count - m), st));
  if (m) {
    hipLaunchKernelGGL(k_dm_hash, dm_grid(m), dim3(DM_BLOCK), 0, st, d->dD, first, (uint32_t)m, d->keys_in, d->vals_in);
    HIPCHK(rocprim::radix_sort_pairs(d->tmp, d->tmp_bytes, (const uint16_t*)d->keys_in, d->keys_out, (const uint32_t*)d->vals_in, d->vals_out, m, 0u, DM_HBITS, st));
    hipLaunchKernelGGL(k_dm_links, dm_grid(m), dim3(DM_BLOCK), 0, st, (const uint16_t*)d->keys_out, (const uint32_t*)d->vals_out, (uint32_t)m,
                       (unsigned)(first & 0xFFFFu), (const uint16_t*)d->head, Lseg);
    hipLaunchKernelGGL(k_dm_heads, dm_grid(m), dim3(DM_BLOCK), 0, st, (const uint16_t*)d->keys_out, (const uint32_t*)d->vals_out, (uint32_t)m,
                       (unsigned)(first & 0xFFFFu), d->head);
  }
  HIPCHK(hipEventRecord(d->ev[k][1], st));
  hipLaunchKernelGGL(k_dm_search_a, dm_grid(count), dim3(DM_BLOCK), 0, st, d->dD, n, (const uint16_t*)d->Lw, first, (uint32_t)count, d->mp[0], d->mp[1], d->Ab);
  HIPCHK(hipEventRecord(d->ev[k][2], st));
  hipLaunchKernelGGL(k_dm_search_b, dm_grid(count), dim3(DM_BLOCK), 0, st, d->dD, n, (const uint16_t*)d->Lw, first, (uint32_t)count, d->mp[0], d->mp[1],
                     (const uint32_t*)d->Ab, d->Bb);
  HIPCHK(hipEventRecord(d->ev[k][3], st));
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  const size_t nbytes = (n - first < count + DM_AHEAD ? n - first : count + DM_AHEAD);
  HIPCHK(hipMemcpyAsync(d->pA(k), d->Ab + 1, 4 * count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(d->pB(k), d->Bb, 4 * count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(d->pL(k), Lseg, 2 * count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(d->pD(k), d->dD + first, nbytes, hipMemcpyDeviceToHost, st));
  if (s + 1 < d->nseg) {  // count == seg >= 32768 here: what the next segment needs of this one
    HIPCHK(hipMemcpyAsync(d->Ab, d->Ab + count, 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(d->Lw, d->Lw + count, 2 * DM_DICT, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipEventRecord(d->ev[k][4], st));
  d->started = s + 1;
  return SP_OK;
}

int32_t sp_deflate_segment_wait(sp_deflate* d, size_t s, size_t* first, size_t* count, const uint8_t** bytes, const uint16_t** L, const uint32_t** A,
                                const uint32_t** B, double* ms) {
  if (!d || s >= d->started || s + 2 < d->started) return SP_EINVAL;
  const int k = (int)(s & 1);
  HIPCHK(hipSetDevice(d->ctx->dev));
  HIPCHK(hipEventSynchronize(d->ev[k][4]));
  if (first) *first = d->first_of(s);
  if (count) *count = d->count_of(s);
  if (bytes) *bytes = d->pD(k);
  if (L) *L = d->pL(k);
  if (A) *A = d->pA(k);
  if (B) *B = d->pB(k);
  if (ms)
    for (int i = 0; i < 4; i++) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, d->ev[k][i], d->ev[k][i + 1]));
      ms[i] = t;
    }
  return SP_OK;
}

int32_t sp_deflate_matches(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, uint16_t* L, uint32_t* A, uint32_t* B) {
  sp_deflate* d = nullptr;
  SPCHK(sp_deflate_open(c, data, n, on_device, probes, &d));
  int32_t rc = SP_OK;
  for (size_t s = 0; s < d->nseg && rc == SP_OK; s++) {
    size_t first = 0, count = 0;
    const uint16_t* l; const uint32_t *a, *b;
    rc = sp_deflate_segment_start(d, s);
    if (rc == SP_OK) rc = sp_deflate_segment_wait(d, s, &first, &count, nullptr, &l, &a, &b, nullptr);
    if (rc != SP_OK) break;
    if (L) memcpy(L + first, l, 2 * count);
    if (A) memcpy(A + first, a, 4 * count);
    if (B) memcpy(B + first, b, 4 * count);
  }
  sp_deflate_close(d);
  return rc;
}

int32_t sp_sparse_bincode(sp_ctx* c, const sp_sparse* const* ms, size_t count, uint64_t num_vars_x, uint64_t num_vars_y, uint8_t* dev_out, size_t cap) {
  if (!c || !ms || !dev_out || ((uintptr_t)dev_out & 7)) return SP_EINVAL;
  size_t need = 0;
  for (size_t k = 0; k < count; k++) {
    if (!ms[k]) return SP_EINVAL;
    need += 24 + 48 * ms[k]->nnz;
  }
  if (cap < need) return SP_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  size_t off = 0;
  for (size_t k = 0; k < count; k++) {
    const sp_sparse* m = ms[k];
    ProfScope ps(c, PF_SPARSE, (4.0 + 4.0 + 32.0 + 48.0) * (double)m->nnz);
    hipLaunchKernelGGL(k_sparse_bincode, dm_grid(3 + 6 * m->nnz), dim3(DM_BLOCK), 0, c->stream, (const uint32_t*)m->ent_row, (const uint32_t*)m->ent_col,
                       (const uint64_t*)m->ent_val, m->nnz, num_vars_x, num_vars_y, (uint64_t*)(dev_out + off));
    off += 24 + 48 * m->nnz;
  }
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  HIPCHK(hipStreamSynchronize(c->stream));
  return SP_OK;
}
}  // extern "C"
