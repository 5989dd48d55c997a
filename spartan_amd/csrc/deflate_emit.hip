// spartan_amd: the coder's share of the device deflate (digest.device = 3), queued per segment behind the parse kernels of deflate_match.hip.
// The parse leaves a compacted token list; tdefl's coder over it comes apart as DESIGN section 7 says (the rules: tdefl_rules.hpp, the host
// model: host/deflate.cc, deflate_blocks_host / BlockPlanner / zlib_from_blocks):
//   the list        list[k] holds, for segment s = k mod 2, the tokens of the block still open at the previous segment's end (at most
//                   DE_CARRY, copied in front of slot DE_CARRY: k_de_carry) followed by the segment's own (rocPRIM select writes them from
//                   slot DE_CARRY on). Where the list begins (l0) and ends is known on the device only; every launch is sized by the bound
//                   cap = DE_CARRY + seg + 1 and reads the true range from device memory.
//   k_de_costs      one lane a slot: code bytes | input bytes << 32 of the token, 0 outside the list; one rocPRIM inclusive scan over cap slots
//   k_de_bounds     one workgroup. The chain from one block start to the next is sequential, each step parallel: the lanes test the block
//                   check on the tokens after the start, 1024 at a time, and take the first TOK_CHECK token at which it fires (the ratio rule
//                   is not monotone: first hit, no bisection). It writes the block records, the list index every block starts at, and the
//                   state the next segment starts from (the open block's first token, its global index and input position).
//   k_de_hist       one workgroup a stretch of the list, cut at block starts: 320 LDS counters, added into the block's record
//   k_de_adler      (sum d, sum (count - i) d) mod 65521 over the segment's bytes; the host combines the pairs
// The records and histograms come down through pinned slot k; the host builds tables, headers and bit offsets (BlockPlanner) and hands them
// up (de_segment_emit), while the device already works on segment s + 1. Then, in workgroups of `chunk` tokens of one block:
//   k_de_len        the chunk's bit length under the block's code sizes (table in LDS)
//   k_de_chunkscan  one lane a block: exclusive scan of its chunks' lengths
//   k_de_emit       a workgroup scan of 256 token lengths at a time on top of the chunk's offset; every token's bits (at most 48) are ORed into
//                   the zeroed output words with atomicOr, which settles the word two tokens, chunks or blocks share; the first chunk of a
//                   block ORs in the header string the host supplied and the end-of-block symbol; a stored block's chunks copy its bytes from
//                   D, whole words plainly and the edge words with atomicOr
// The compressed bytes stay resident (they are the result, at most the input's size and a header a block: see DESIGN section 3) and come down
// once. Every index is bounded: list slots by cap, block slots by maxblk (a segment that would close more sets the error flag and stops),
// output words by out_words (a write past it is dropped; the host has sized the buffer by the stream's bound and checks the length).
#include <rocprim/block/block_scan.hpp>
#include <rocprim/device/device_scan.hpp>

#include "deflate_emit.hpp"
#include "internal.hpp"
#include "tdefl_rules.hpp"

namespace {
constexpr unsigned DE_BLOCK = 256, DE_BOUNDS = 1024, DE_STRETCH = 4096, DE_ADLER_TILE = 4096;
constexpr uint32_t DE_NONE = 0xFFFFFFFFu;
constexpr uint32_t DE_KIND_STORED = 2;

struct DeState { uint32_t l0, src_first; uint64_t gtok, pos; };  // a segment's start: its list begins at l0 with prev list's src_first
struct DeOut { uint32_t nblk, err; unsigned long long adler[2]; };

__global__ void __launch_bounds__(DE_BLOCK) k_de_carry(const uint32_t* __restrict__ prev, uint32_t* __restrict__ cur, const DeState* __restrict__ st) {
  const uint32_t i = blockIdx.x * DE_BLOCK + threadIdx.x, l0 = st->l0;
  if (l0 > DE_CARRY || i >= DE_CARRY - l0) return;
  cur[l0 + i] = prev[st->src_first + i];
}
__device__ __forceinline__ uint32_t de_list_end(const size_t* ntok, uint32_t cap) {
  const size_t k = *ntok;
  return DE_CARRY + (uint32_t)(k < cap - DE_CARRY ? k : cap - DE_CARRY);
}
__global__ void __launch_bounds__(DE_BLOCK) k_de_costs(const uint32_t* __restrict__ list, const size_t* __restrict__ ntok, const DeState* __restrict__ st,
                                                       uint32_t cap, uint64_t* __restrict__ cost) {
  const uint32_t i = blockIdx.x * DE_BLOCK + threadIdx.x;
  if (i >= cap) return;
  uint64_t c = 0;
  if (i >= st->l0 && i < de_list_end(ntok, cap)) {
    const uint32_t t = list[i];
    c = tdefl::tok_code_bytes(t) | ((uint64_t)tdefl::tok_input_bytes(t) << 32);
  }
  cost[i] = c;
}
// rec: 8 words a block: first token's global index (lo, hi), tokens, input bytes, rule, lookahead_pos - lz_dict_pos, dict_size, 0
__global__ void __launch_bounds__(DE_BOUNDS) k_de_bounds(const uint32_t* __restrict__ list, const uint64_t* __restrict__ scan, const size_t* __restrict__ ntok,
                                                         const DeState* __restrict__ in, DeState* __restrict__ next, uint32_t cap, uint64_t n, int last,
                                                         uint32_t maxblk, uint32_t* __restrict__ rec, uint32_t* __restrict__ bstart, DeOut* __restrict__ out) {
  __shared__ uint32_t s_hit;
  const uint32_t tid = threadIdx.x, l0 = in->l0 <= DE_CARRY ? in->l0 : DE_CARRY, end = de_list_end(ntok, cap);
  uint32_t start = l0, nb = 0, err = 0;
  uint64_t base = 0;  // the sums in front of the block under way (slots before l0 cost nothing)
  auto record = [&](uint32_t e, uint32_t rule) {  // lane 0: the block list[start, e)
    const uint32_t k = e - start;
    const uint64_t total = k ? (scan[e - 1] - base) >> 32 : 0, at0 = in->pos + (base >> 32);
    uint64_t la = 0;
    uint32_t ds = 0;
    if (k) {
      const uint32_t t = list[e - 1];
      tdefl::tok_step(t, at0 + total - tdefl::tok_input_bytes(t), n, &la, &ds);
      la -= at0;
    }
    const uint64_t g = in->gtok + (start - l0);
    uint32_t* r = rec + 8 * (size_t)nb;
    r[0] = (uint32_t)g; r[1] = (uint32_t)(g >> 32); r[2] = k; r[3] = (uint32_t)total; r[4] = rule; r[5] = (uint32_t)la; r[6] = ds; r[7] = 0;
    bstart[nb] = start;
  };
  for (;;) {
    uint32_t hit = DE_NONE;
    for (uint32_t w = start; w < end; w += DE_BOUNDS) {
      if (tid == 0) s_hit = DE_NONE;
      __syncthreads();
      const uint32_t i = w + tid;
      if (i < end && (list[i] & tdefl::TOK_CHECK)) {
        const uint64_t d = scan[i] - base;
        if (tdefl::block_check(tdefl::code_bytes_after(d & 0xFFFFFFFFu, i - start + 1), d >> 32) != tdefl::RULE_NONE) atomicMin(&s_hit, i);
      }
      __syncthreads();
      hit = s_hit;
      __syncthreads();
      if (hit != DE_NONE) break;
    }
    if (hit == DE_NONE) break;
    if (nb >= maxblk) { err = 1; break; }
    if (tid == 0) {
      const uint64_t d = scan[hit] - base;
      record(hit + 1, tdefl::block_check(tdefl::code_bytes_after(d & 0xFFFFFFFFu, hit - start + 1), d >> 32));
    }
    base = scan[hit]; start = hit + 1; nb++;
  }
  if (last && !err) {
    if (nb >= maxblk) err = 1;
    else {
      if (tid == 0) record(end, tdefl::RULE_FINISH);
      if (end > start) base = scan[end - 1];
      start = end; nb++;
    }
  }
  uint32_t open = end - start;
  if (open > DE_CARRY) { err = 2; open = 0; }
  if (tid == 0) {
    bstart[nb] = start;
    next->l0 = DE_CARRY - open; next->src_first = start; next->gtok = in->gtok + (start - l0); next->pos = in->pos + (base >> 32);
    out->nblk = err ? 0 : nb; out->err = err;
  }
}
__device__ __forceinline__ void de_count(uint32_t t, uint32_t* cnt) {
  const unsigned len = tdefl::tok_len(t);
  if (!len) { atomicAdd(&cnt[t & 0xFF], 1u); return; }
  unsigned s, ne, ev;
  tdefl::len_symbol(len, &s, &ne, &ev);
  atomicAdd(&cnt[s], 1u);
  tdefl::dist_symbol(tdefl::tok_dist(t), &s, &ne, &ev);
  atomicAdd(&cnt[288 + s], 1u);
}
__global__ void __launch_bounds__(DE_BLOCK) k_de_hist(const uint32_t* __restrict__ list, const uint32_t* __restrict__ bstart, const DeOut* __restrict__ out,
                                                      uint32_t cap, uint32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[tdefl::TABLE_WORDS];
  const uint32_t nb = out->nblk, r0 = blockIdx.x * DE_STRETCH, r1 = r0 + DE_STRETCH < cap ? r0 + DE_STRETCH : cap;
  for (uint32_t b = 0; b < nb; b++) {
    const uint32_t bs = bstart[b], be = bstart[b + 1];
    const uint32_t lo = bs > r0 ? bs : r0, hi = be < r1 ? be : r1;
    if (lo >= hi) continue;  // the same for every lane
    for (uint32_t j = threadIdx.x; j < tdefl::TABLE_WORDS; j += DE_BLOCK) cnt[j] = 0;
    __syncthreads();
    for (uint32_t i = lo + threadIdx.x; i < hi; i += DE_BLOCK) de_count(list[i], cnt);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < tdefl::TABLE_WORDS; j += DE_BLOCK)
      if (cnt[j]) atomicAdd(&hist[(size_t)b * tdefl::TABLE_WORDS + j], cnt[j]);
    __syncthreads();
  }
}
__global__ void __launch_bounds__(DE_BLOCK) k_de_adler(const uint8_t* __restrict__ seg, uint32_t count, DeOut* __restrict__ out) {
  __shared__ unsigned long long acc[2];
  if (threadIdx.x < 2) acc[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long a = 0, b = 0;
  const uint32_t t0 = blockIdx.x * DE_ADLER_TILE;
  for (uint32_t j = threadIdx.x; j < DE_ADLER_TILE; j += DE_BLOCK) {
    const uint32_t i = t0 + j;
    if (i < count) { const unsigned d = seg[i]; a += d; b += (unsigned long long)(count - i) * d; }
  }
  atomicAdd(&acc[0], a); atomicAdd(&acc[1], b);
  __syncthreads();
  if (threadIdx.x < 2) atomicAdd(&out->adler[threadIdx.x], acc[threadIdx.x] % 65521u);
}

// ---- the emission. plans: 8 words a block: bit_off, hdr_bits, kind, tok_off, eob_off, src, total, 0; chunk0[b]: the block's first chunk
__device__ __forceinline__ uint32_t de_block_of(const uint32_t* __restrict__ chunk0, uint32_t nblk, uint32_t c) {
  uint32_t lo = 0, hi = nblk;  // the last b with chunk0[b] <= c
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (chunk0[mid] <= c) lo = mid; else hi = mid; }
  return lo;
}
__device__ __forceinline__ void de_or_bits(uint32_t* __restrict__ out, size_t out_words, uint64_t off, uint64_t v, unsigned nb) {
  if (!nb) return;
  const size_t w = off >> 5;
  const unsigned sh = (unsigned)(off & 31);
  const uint32_t w0 = (uint32_t)v << sh;
  const uint64_t rest = sh ? v >> (32 - sh) : v >> 32;
  const uint32_t w1 = (uint32_t)rest, w2 = (uint32_t)(rest >> 32);
  if (w0 && w < out_words) atomicOr(&out[w], w0);
  if (w1 && w + 1 < out_words) atomicOr(&out[w + 1], w1);
  if (w2 && w + 2 < out_words) atomicOr(&out[w + 2], w2);
}
__global__ void __launch_bounds__(DE_BLOCK) k_de_len(const uint32_t* __restrict__ list, const uint32_t* __restrict__ bstart, const uint64_t* __restrict__ plans,
                                                     const uint32_t* __restrict__ tables, const uint32_t* __restrict__ chunk0, uint32_t nblk, uint32_t chunk,
                                                     uint32_t* __restrict__ chunksum) {
  __shared__ uint32_t tab[tdefl::TABLE_WORDS];
  __shared__ uint32_t sum;
  const uint32_t c = blockIdx.x, b = de_block_of(chunk0, nblk, c), j = c - chunk0[b];
  for (uint32_t i = threadIdx.x; i < tdefl::TABLE_WORDS; i += DE_BLOCK) tab[i] = tables[(size_t)b * tdefl::TABLE_WORDS + i];
  if (threadIdx.x == 0) sum = 0;
  __syncthreads();
  uint32_t mine = 0;
  if (plans[8 * (size_t)b + 2] != DE_KIND_STORED) {
    const uint32_t be = bstart[b + 1];
    const uint64_t t0 = (uint64_t)bstart[b] + (uint64_t)j * chunk, t1 = t0 + chunk < be ? t0 + chunk : be;
    for (uint64_t i = t0 + threadIdx.x; i < t1; i += DE_BLOCK) mine += tdefl::tok_nbits(list[i], tab);
  }
  if (mine) atomicAdd(&sum, mine);
  __syncthreads();
  if (threadIdx.x == 0) chunksum[c] = sum;
}
__global__ void __launch_bounds__(64) k_de_chunkscan(const uint32_t* __restrict__ chunk0, uint32_t nblk, uint32_t* __restrict__ chunksum) {
  const uint32_t b = blockIdx.x * 64 + threadIdx.x;
  if (b >= nblk) return;
  uint32_t run = 0;
  for (uint32_t c = chunk0[b]; c < chunk0[b + 1]; c++) { const uint32_t t = chunksum[c]; chunksum[c] = run; run += t; }
}
__global__ void __launch_bounds__(DE_BLOCK) k_de_emit(const uint32_t* __restrict__ list, const uint32_t* __restrict__ bstart, const uint64_t* __restrict__ plans,
                                                      const uint32_t* __restrict__ tables, const uint8_t* __restrict__ hdrs, const uint32_t* __restrict__ chunk0,
                                                      uint32_t nblk, uint32_t chunk, const uint32_t* __restrict__ chunksum, const uint8_t* __restrict__ D, uint64_t n,
                                                      uint32_t* __restrict__ out, size_t out_words) {
  using Scan = rocprim::block_scan<uint32_t, DE_BLOCK>;
  __shared__ typename Scan::storage_type scan_lds;
  __shared__ uint32_t tab[tdefl::TABLE_WORDS];
  const uint32_t c = blockIdx.x, b = de_block_of(chunk0, nblk, c), j = c - chunk0[b], tid = threadIdx.x;
  const uint64_t* p = plans + 8 * (size_t)b;
  const uint64_t bit_off = p[0], tok_off = p[3];
  const uint32_t hdr_bits = (uint32_t)p[1], kind = (uint32_t)p[2];
  for (uint32_t i = tid; i < tdefl::TABLE_WORDS; i += DE_BLOCK) tab[i] = tables[(size_t)b * tdefl::TABLE_WORDS + i];
  __syncthreads();
  if (j == 0) {  // the header string, a byte a lane; the end-of-block symbol
    const uint32_t hb = hdr_bits < 8 * DE_HDR_BYTES ? hdr_bits : 8 * (uint32_t)DE_HDR_BYTES;
    for (uint32_t i = tid; 8 * i < hb; i += DE_BLOCK) de_or_bits(out, out_words, bit_off + 8 * i, hdrs[(size_t)b * DE_HDR_BYTES + i], hb - 8 * i < 8 ? hb - 8 * i : 8);
    if (tid == 0 && kind != DE_KIND_STORED) de_or_bits(out, out_words, p[4], tab[256] & 0xFFFF, tab[256] >> 16);
  }
  if (kind == DE_KIND_STORED) {  // destination words [w0, w1) cut evenly among the block's chunks, a word a lane
    const uint64_t src = p[5], total = p[6], db = tok_off >> 3;
    if (src + total > n) return;
    const uint64_t w0 = db >> 2, w1 = (db + total + 3) >> 2, nch = chunk0[b + 1] - chunk0[b], per = (w1 - w0 + nch - 1) / nch;
    const uint64_t a = w0 + j * per, e = a + per < w1 ? a + per : w1;
    for (uint64_t w = a + tid; w < e; w += DE_BLOCK) {
      uint32_t v = 0;
      bool whole = true;
      for (unsigned k = 0; k < 4; k++) {
        const uint64_t q = 4 * w + k;  // a byte of the stream
        if (q >= db && q < db + total) v |= (uint32_t)D[src + (q - db)] << (8 * k); else whole = false;
      }
      if (w >= out_words) continue;
      if (whole) out[w] = v; else if (v) atomicOr(&out[w], v);
    }
    return;
  }
  const uint32_t be = bstart[b + 1];
  const uint64_t t0 = (uint64_t)bstart[b] + (uint64_t)j * chunk, t1 = t0 + chunk < be ? t0 + chunk : be;
  uint64_t at = tok_off + chunksum[c];
  for (uint64_t r = t0; r < t1; r += DE_BLOCK) {  // the same trip count for every lane
    const uint64_t i = r + tid;
    uint64_t v = 0;
    uint32_t nb = 0, before = 0, all = 0;
    if (i < t1) nb = tdefl::tok_bits(list[i], tab, &v);
    Scan().exclusive_scan(nb, before, 0u, all, scan_lds);
    de_or_bits(out, out_words, at + before, v, nb);
    at += all;
    __syncthreads();
  }
}
static inline dim3 de_grid(size_t n, unsigned per) { return dim3((unsigned)((n + per - 1) / per)); }
}  // namespace

struct DeEmit {
  hipStream_t st = nullptr;
  const uint8_t* dD = nullptr;
  size_t n = 0, seg = 0, nseg = 0;
  uint32_t cap = 0, maxblk = 0, chunk = 0, maxchunks = 0;
  uint32_t* list[2] = {nullptr, nullptr};
  uint32_t* bstart[2] = {nullptr, nullptr};
  size_t* ntok = nullptr;  // [2]
  uint64_t *cost = nullptr, *scan = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  DeState* state = nullptr;  // [nseg + 1]
  uint8_t* res = nullptr;    // [DeOut, padded to 32][rec: 32 maxblk][hist: 1280 maxblk], copied down in one piece
  size_t res_bytes = 0;
  uint8_t* down[2] = {nullptr, nullptr};  // pinned: res as segment k left it
  uint8_t* up[2] = {nullptr, nullptr};    // pinned: [plans: 64 maxblk][chunk0: 4 (maxblk + 1), padded][tables: 1280 maxblk][hdrs: 320 maxblk]
  uint8_t* dup = nullptr;                 // its place on the device
  size_t up_chunk0 = 0, up_tables = 0, up_hdrs = 0, up_bytes = 0;
  uint32_t* chunksum = nullptr;
  uint32_t* out = nullptr;  // the compressed stream, zeroed: resident until de_bytes
  size_t out_words = 0;
  hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  bool timed[2] = {false, false};
  double ms_emit = 0;
  std::vector<uint64_t> rec64;
  std::vector<uint16_t> hist16;
};

void de_close(DeEmit* e) {
  if (!e) return;
  for (auto& pair : e->ev)
    for (hipEvent_t v : pair)
      if (v) (void)hipEventDestroy(v);
  for (void* p : {(void*)e->down[0], (void*)e->down[1], (void*)e->up[0], (void*)e->up[1]})
    if (p) (void)hipHostFree(p);
  for (void* p : {(void*)e->list[0], (void*)e->list[1], (void*)e->bstart[0], (void*)e->bstart[1], (void*)e->ntok, (void*)e->cost, (void*)e->scan, e->tmp,
                  (void*)e->state, (void*)e->res, (void*)e->dup, (void*)e->chunksum, (void*)e->out})
    if (p) (void)hipFree(p);
  delete e;
}

static int32_t de_alloc(DeEmit* e) {
  const size_t cap = e->cap, maxblk = e->maxblk;
  for (int k = 0; k < 2; k++) {
    HIPCHK(hipMalloc((void**)&e->list[k], 4 * cap));
    HIPCHK(hipMalloc((void**)&e->bstart[k], 4 * (maxblk + 1)));
    HIPCHK(hipHostMalloc((void**)&e->down[k], e->res_bytes, hipHostMallocDefault));
    HIPCHK(hipHostMalloc((void**)&e->up[k], e->up_bytes, hipHostMallocDefault));
    for (hipEvent_t& v : e->ev[k]) HIPCHK(hipEventCreate(&v));
  }
  HIPCHK(hipMalloc((void**)&e->ntok, 2 * sizeof(size_t)));
  HIPCHK(hipMalloc((void**)&e->cost, 8 * cap));
  HIPCHK(hipMalloc((void**)&e->scan, 8 * cap));
  HIPCHK(rocprim::inclusive_scan(nullptr, e->tmp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, cap, rocprim::plus<uint64_t>(), e->st));
  HIPCHK(hipMalloc(&e->tmp, e->tmp_bytes ? e->tmp_bytes : 256));
  HIPCHK(hipMalloc((void**)&e->state, sizeof(DeState) * (e->nseg + 1)));
  HIPCHK(hipMalloc((void**)&e->res, e->res_bytes));
  HIPCHK(hipMalloc((void**)&e->dup, e->up_bytes));
  HIPCHK(hipMalloc((void**)&e->chunksum, 4 * (size_t)e->maxchunks));
  HIPCHK(hipMalloc((void**)&e->out, 4 * e->out_words));
  HIPCHK(hipMemsetAsync(e->out, 0, 4 * e->out_words, e->st));
  HIPCHK(hipMemsetAsync(e->state, 0, sizeof(DeState) * (e->nseg + 1), e->st));
  const DeState first{DE_CARRY, DE_CARRY, 0, 0};
  HIPCHK(hipMemcpyAsync(e->state, &first, sizeof first, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipStreamSynchronize(e->st));  // `first` leaves the stack
  return SP_OK;
}
int32_t de_open(DeEmit** out, hipStream_t st, const uint8_t* dD, size_t n, size_t seg, size_t nseg, size_t chunk) {
  if (!chunk) chunk = 4096;
  if (chunk < 256 || chunk > 65536 || seg + 1 + DE_CARRY >= 0xFFFFFFFFull) return SP_EINVAL;
  DeEmit* e = new (std::nothrow) DeEmit();
  if (!e) return SP_ENOMEM;
  e->st = st; e->dD = dD; e->n = n; e->seg = seg; e->nseg = nseg; e->chunk = (uint32_t)chunk;
  e->cap = (uint32_t)(DE_CARRY + seg + 1);
  e->maxblk = (uint32_t)de_max_blocks(e->cap);
  e->maxchunks = (uint32_t)(e->cap / chunk + e->maxblk + 1);
  e->res_bytes = 32 + (32 + 4 * DE_HIST) * (size_t)e->maxblk;
  e->up_chunk0 = 64 * (size_t)e->maxblk;
  e->up_tables = e->up_chunk0 + (4 * ((size_t)e->maxblk + 1) + 7) / 8 * 8;
  e->up_hdrs = e->up_tables + 4 * DE_HIST * (size_t)e->maxblk;
  e->up_bytes = e->up_hdrs + DE_HDR_BYTES * (size_t)e->maxblk;
  // the stream's bound: the input, half as much again for blocks that can neither be stored nor shrink, a header a block, head and trailer
  e->out_words = (n + n / 2 + 512 * de_max_blocks(n) + 64) / 4 + 4;
  const int32_t rc = de_alloc(e);
  if (rc != SP_OK) { de_close(e); e = nullptr; }
  *out = e;
  return rc;
}
uint32_t* de_tokens(DeEmit* e, size_t s) { return e->list[s & 1] + DE_CARRY; }
size_t* de_ntok(DeEmit* e, size_t s) { return e->ntok + (s & 1); }

int32_t de_segment_blocks(DeEmit* e, size_t s, size_t first, size_t count) {
  const int k = (int)(s & 1);
  hipStream_t st = e->st;
  const uint32_t cap = e->cap;
  DeOut* out = (DeOut*)e->res;
  uint32_t* rec = (uint32_t*)(e->res + 32);
  uint32_t* hist = (uint32_t*)(e->res + 32 + 32 * (size_t)e->maxblk);
  HIPCHK(hipMemsetAsync(e->res, 0, e->res_bytes, st));
  hipLaunchKernelGGL(k_de_carry, de_grid(DE_CARRY, DE_BLOCK), dim3(DE_BLOCK), 0, st, (const uint32_t*)e->list[k ^ 1], e->list[k], (const DeState*)e->state + s);
  hipLaunchKernelGGL(k_de_costs, de_grid(cap, DE_BLOCK), dim3(DE_BLOCK), 0, st, (const uint32_t*)e->list[k], (const size_t*)e->ntok + k,
                     (const DeState*)e->state + s, cap, e->cost);
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  HIPCHK(rocprim::inclusive_scan(e->tmp, e->tmp_bytes, (const uint64_t*)e->cost, e->scan, (size_t)cap, rocprim::plus<uint64_t>(), st));
  hipLaunchKernelGGL(k_de_bounds, dim3(1), dim3(DE_BOUNDS), 0, st, (const uint32_t*)e->list[k], (const uint64_t*)e->scan, (const size_t*)e->ntok + k,
                     (const DeState*)e->state + s, e->state + s + 1, cap, (uint64_t)e->n, s + 1 == e->nseg ? 1 : 0, e->maxblk, rec, e->bstart[k], out);
  hipLaunchKernelGGL(k_de_hist, de_grid(cap, DE_STRETCH), dim3(DE_BLOCK), 0, st, (const uint32_t*)e->list[k], (const uint32_t*)e->bstart[k], (const DeOut*)out, cap,
                     hist);
  hipLaunchKernelGGL(k_de_adler, de_grid(count, DE_ADLER_TILE), dim3(DE_BLOCK), 0, st, e->dD + first, (uint32_t)count, out);
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  HIPCHK(hipMemcpyAsync(e->down[k], e->res, e->res_bytes, hipMemcpyDeviceToHost, st));
  return SP_OK;
}

int32_t de_blocks(DeEmit* e, size_t s, size_t* nblocks, const uint64_t** records, const uint16_t** hist, uint64_t adler[2]) {
  const uint8_t* r = e->down[s & 1];
  const DeOut* o = (const DeOut*)r;
  if (o->err || o->nblk > e->maxblk) return SP_EINVAL;  // more blocks, or a longer open block, than tdefl's rules allow: never
  const uint32_t* rec = (const uint32_t*)(r + 32);
  const uint32_t* h = (const uint32_t*)(r + 32 + 32 * (size_t)e->maxblk);
  e->rec64.resize(DE_REC_WORDS * (size_t)o->nblk + 1);
  e->hist16.resize(DE_HIST * (size_t)o->nblk + 1);
  for (size_t b = 0; b < o->nblk; b++) {
    const uint32_t* q = rec + 8 * b;
    uint64_t* d = e->rec64.data() + DE_REC_WORDS * b;
    d[0] = q[0] | ((uint64_t)q[1] << 32); d[1] = q[2]; d[2] = q[3]; d[3] = q[4]; d[4] = q[5]; d[5] = q[6];
    for (size_t i = 0; i < DE_HIST; i++) e->hist16[DE_HIST * b + i] = (uint16_t)h[DE_HIST * b + i];  // a block has at most 58249 tokens
  }
  if (nblocks) *nblocks = o->nblk;
  if (records) *records = e->rec64.data();
  if (hist) *hist = e->hist16.data();
  if (adler) { adler[0] = o->adler[0] % 65521u; adler[1] = o->adler[1] % 65521u; }
  return SP_OK;
}

int32_t de_segment_emit(DeEmit* e, size_t s, size_t nblocks, const uint64_t* plans, const uint32_t* tables, const uint8_t* hdrs) {
  const int k = (int)(s & 1);
  const DeOut* o = (const DeOut*)e->down[k];
  if (nblocks != o->nblk || (nblocks && (!plans || !tables || !hdrs))) return SP_EINVAL;
  if (!nblocks) return SP_OK;
  hipStream_t st = e->st;
  if (e->timed[k]) {  // the emission that used this slot's events two segments ago is behind the records just waited for
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, e->ev[k][0], e->ev[k][1]));
    e->ms_emit += t; e->timed[k] = false;
  }
  const uint32_t* rec = (const uint32_t*)(e->down[k] + 32);
  uint8_t* up = e->up[k];
  uint64_t* pl = (uint64_t*)up;
  uint32_t* chunk0 = (uint32_t*)(up + e->up_chunk0);
  uint32_t nch = 0;
  for (size_t b = 0; b < nblocks; b++) {
    const uint64_t* p = plans + DE_PLAN_WORDS * b;  // bit_off, hdr_bits, kind, tok_off, eob_off, src
    const uint32_t ntok = rec[8 * b + 2];
    pl[8 * b + 0] = p[0]; pl[8 * b + 1] = p[1]; pl[8 * b + 2] = p[2]; pl[8 * b + 3] = p[3]; pl[8 * b + 4] = p[4]; pl[8 * b + 5] = p[5];
    pl[8 * b + 6] = rec[8 * b + 3]; pl[8 * b + 7] = 0;
    if (p[1] > 8 * DE_HDR_BYTES || p[2] > DE_KIND_STORED) return SP_EINVAL;
    chunk0[b] = nch;
    nch += ntok ? (ntok + e->chunk - 1) / e->chunk : 1;  // an empty block still has a header and an end-of-block symbol to write
  }
  chunk0[nblocks] = nch;
  if (nch > e->maxchunks) return SP_EINVAL;
  memcpy(up + e->up_tables, tables, 4 * DE_HIST * nblocks);
  memcpy(up + e->up_hdrs, hdrs, DE_HDR_BYTES * nblocks);
  HIPCHK(hipMemcpyAsync(e->dup, up, e->up_bytes, hipMemcpyHostToDevice, st));
  const uint64_t* dpl = (const uint64_t*)e->dup;
  const uint32_t* dch = (const uint32_t*)(e->dup + e->up_chunk0);
  const uint32_t* dtab = (const uint32_t*)(e->dup + e->up_tables);
  const uint8_t* dhdr = e->dup + e->up_hdrs;
  const uint32_t nb = (uint32_t)nblocks;
  HIPCHK(hipEventRecord(e->ev[k][0], st));
  hipLaunchKernelGGL(k_de_len, dim3(nch), dim3(DE_BLOCK), 0, st, (const uint32_t*)e->list[k], (const uint32_t*)e->bstart[k], dpl, dtab, dch, nb, e->chunk, e->chunksum);
  hipLaunchKernelGGL(k_de_chunkscan, dim3((nb + 63) / 64), dim3(64), 0, st, dch, nb, e->chunksum);
  hipLaunchKernelGGL(k_de_emit, dim3(nch), dim3(DE_BLOCK), 0, st, (const uint32_t*)e->list[k], (const uint32_t*)e->bstart[k], dpl, dtab, dhdr, dch, nb, e->chunk,
                     (const uint32_t*)e->chunksum, e->dD, (uint64_t)e->n, e->out, e->out_words);
  if (hipGetLastError() != hipSuccess) return SP_EHIP;
  HIPCHK(hipEventRecord(e->ev[k][1], st));
  e->timed[k] = true;
  return SP_OK;
}

int32_t de_bytes(DeEmit* e, uint8_t* out, size_t nbytes, double* ms) {
  if (nbytes > 4 * e->out_words || (nbytes && !out)) return SP_EINVAL;
  HIPCHK(hipStreamSynchronize(e->st));
  for (int k = 0; k < 2; k++)
    if (e->timed[k]) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, e->ev[k][0], e->ev[k][1]));
      e->ms_emit += t; e->timed[k] = false;
    }
  if (nbytes) HIPCHK(hipMemcpy(out, e->out, nbytes, hipMemcpyDeviceToHost));
  if (ms) *ms = e->ms_emit;
  return SP_OK;
}
