// spartan_amd: the device's share of R1CSShape::get_digest (src/r1cs.rs:154-158). The digest is the zlib stream of bincode(shape) as miniz's
// tdefl writes it at level 6 (spartan_amd/host/deflate.cc restates tdefl). Two things run here:
//   sp_sparse_bincode    the matrices' part of bincode(R1CSShape), serialised from the resident entries into a device byte buffer
//   sp_deflate_*         tdefl's hash-chain match search, one input position per lane; and, for a handle opened by sp_deflate_open_parse,
//                        tdefl's lazy PARSE over the tables it fills, so that the host receives tokens instead of tables
// The block decisions and the Huffman coding stay on the host (deflate.cc: MatchParser over tables, TokenCoder over tokens), unless the handle
// was opened by sp_deflate_open_emit: then the coder's block boundaries, histograms and bit emission are queued behind the parse
// (deflate_emit.hip) and the host keeps the Huffman tables and bit offsets alone.
// tdefl's rules themselves — hash, probe budget, find, the candidate filter, walk, the token word — are tdefl_rules.hpp, which the host runs
// too; this file holds the kernels that apply them a position per lane, and the segment pipeline around them.
//
// The search, per position p of the input D[0, n):
//   links   L[p] = low 16 bits of the greatest q < p with hash3(q) == hash3(p), else 0. Within a segment: a stable radix sort of the
//           positions by hash (rocPRIM); an element takes the position before it in its group, the first of a group takes the head carried
//           from the segments before; the last of a group becomes the new head.
//   A[p] = find(p, 2);  B[p] = find(p, len(A[p-1])) where A[p-1] leaves the parser's filter as a held match.
// A segment needs of its predecessors: head[32768], the last 32768 links, A[first - 1]. The link window Lw holds L[first - 32768, first +
// count), so find's Lfirst is first - 32768 (modulo 2^64 in segment 0, whose first 32768 slots no search reaches): window index
// cand - first + 32768 with cand >= p - 32768 + lookahead >= first - 32768.
//
// The parse: from a free state at p everything up to the next free state F(p) is a function of D, A, B and, for the rare look-up neither
// table answers, find; 1 <= F(p) - p <= 383 (tdefl_rules.hpp, walk). The tokens are those of the walks from the positions REACHABLE from
// the segment's entry under F. Per segment of `count` positions, tiles of T and groups of G tiles (DP_HEAD = 384 <= T, so a jump never
// skips a tile and enters one within its first 384 positions):
//   k_dp_jump     one lane a position: delta[i] = F(i) - i by the walk itself, nothing written but the 16-bit delta (a walk stops at the
//                 segment's end as the parser's loop does: delta then reaches exactly `count`, with a match still held)
//   k_dp_exit     one workgroup a tile: pointer doubling in LDS, log2(T) + 1 rounds, gives every position of the tile its exit, the first
//                 position at or past the tile's end; kept for the tile's first 384 positions: X0
//   k_dp_compose  one lane for each of a group's first 384 positions: G dependent steps through X0 give the group's exit: X1
//   k_dp_top      one lane: the segment's prologue (an entry that holds a match is resolved from the carried state, its tokens written),
//                 then the walk over the groups through X1, leaving each group's entry
//   k_dp_down     one lane a group: G steps through X0 leave each tile's entry
//   k_dp_mark     one lane a tile: the walk over delta[] from the tile's entry sets bit 15 of every reachable position's delta
//   k_dp_tokens   one lane a position: a marked one redoes its walk and writes its tokens, one word per position (0: no token starts
//                 here; slot 0 stands for position first - 1, where the prologue's token starts); the walk that reaches the segment's end
//                 writes the state the next segment enters with
//   rocPRIM select  the nonzero words, in order, into the pinned slot, with their number
// Scratch per position of one segment: about 30 bytes of the search, plus 2 of jumps, 4 of token words and 1536 / T of exits: about 38; the
// pinned slots hold 5 bytes a position (token words and the bytes) instead of 11.
// The longest dependent chain is log2(T) + 3 G + count / (T G) + T steps instead of `count`. Every index is bounded: a walk looks up only
// positions below first + count; delta, tok (count + 1 words) and the marks are indexed by positions < count; X0 / X1 by (tile or group,
// offset < 384) with offset = position - start of the tile or group it lies in, which a jump of at most 383 from before that start keeps
// below 384.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "deflate_emit.hpp"
#include "internal.hpp"
#include "tdefl_rules.hpp"

namespace {
constexpr unsigned DM_BLOCK = 256;       // one position per lane, four wavefronts a workgroup
constexpr unsigned DM_DICT = tdefl::DICT;
constexpr size_t DM_AHEAD = tdefl::MAXM;  // bytes past a segment's end its parser reads (the lookahead of its last position)

// keys[i] = hash3(first + i), vals[i] = i for the m positions of the segment that have three bytes
__global__ void __launch_bounds__(DM_BLOCK) k_dm_hash(const uint8_t* __restrict__ D, size_t first, uint32_t m, uint16_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= m) return;
  keys[i] = (uint16_t)tdefl::hash3(D + first + i);
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

// Lw[q - first + 32768] = L[q];  Ab[0] = A[first - 1] (0 before the first position), Ab[1 + i] = A[first + i];  Bb[i] = B[first + i]
__global__ void __launch_bounds__(DM_BLOCK) k_dm_search_a(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, size_t first, uint32_t count,
                                                          unsigned mp0, unsigned mp1, uint32_t* __restrict__ Ab) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= count) return;
  const unsigned mp[2] = {mp0, mp1};
  Ab[1 + i] = tdefl::find(D, n, Lw, first - DM_DICT, first + i, tdefl::MINM - 1, mp);
}
__global__ void __launch_bounds__(DM_BLOCK) k_dm_search_b(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, size_t first, uint32_t count,
                                                          unsigned mp0, unsigned mp1, const uint32_t* __restrict__ Ab, uint32_t* __restrict__ Bb) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= count) return;
  const size_t p = first + i;
  const uint32_t a = Ab[i];
  const unsigned mp[2] = {mp0, mp1};
  Bb[i] = (p && tdefl::held(a, p - 1)) ? tdefl::find(D, n, Lw, first - DM_DICT, p, a >> 16, mp) : 0u;
}

// ---- the parse: walks between free states
constexpr uint32_t DP_HEAD = 384;                    // 1 + the longest jump: the positions of a tile a walk from before it can enter at
constexpr uint32_t DP_MARK = 0x8000u;
struct DpCarry { uint32_t entry, sl, sd, fallbacks; };  // a segment's entry: position relative to its first, the held match (sl == 0: free)
// tdefl::walk from the state (first + q, sl, sd) over the segment's tables: the look-up is A when free, B when A[p - 1] is held at exactly
// this length, else searched on the spot; tok[1 + i] is position first + i's word. Returns the next step's position relative to `first`
// (> count when a match crosses the segment's end); sl, sd: the match then held.
template <bool EMIT>
__device__ __forceinline__ uint32_t dp_segment_walk(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, const uint32_t* __restrict__ Ab,
                                                    const uint32_t* __restrict__ Bb, size_t first, uint32_t count, uint32_t q, unsigned& sl, unsigned& sd,
                                                    unsigned mp0, unsigned mp1, uint32_t* __restrict__ tok, unsigned& fallbacks) {
  const unsigned mp[2] = {mp0, mp1};
  tdefl::WalkState w{first + q, sl, sd};
  tdefl::walk(
      D, w, first + count,
      [&](size_t p, unsigned init) -> uint32_t {
        const size_t i = p - first;
        if (init == tdefl::MINM - 1) return Ab[1 + i];
        const uint32_t a = Ab[i];  // A[p - 1]
        if (tdefl::held(a, p - 1) && (a >> 16) == init) return Bb[i];
        fallbacks++;
        return tdefl::find(D, n, Lw, first - DM_DICT, p, init, mp);
      },
      [&](size_t pos, uint32_t t) {
        if (EMIT) tok[1 + pos - first] = t;
      });
  sl = w.sl; sd = w.sd;
  return (uint32_t)(w.q - first);
}
__global__ void __launch_bounds__(DM_BLOCK) k_dp_jump(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, const uint32_t* __restrict__ Ab,
                                                      const uint32_t* __restrict__ Bb, size_t first, uint32_t count, unsigned mp0, unsigned mp1,
                                                      uint16_t* __restrict__ delta) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= count) return;
  unsigned sl = 0, sd = 0, fb = 0;
  const uint32_t next = dp_segment_walk<false>(D, n, Lw, Ab, Bb, first, count, i, sl, sd, mp0, mp1, nullptr, fb);
  delta[i] = (uint16_t)(next - i);  // 1 .. 383
}
// dynamic LDS: two arrays of T 16-bit tile-relative targets (< T + 384)
__global__ void __launch_bounds__(DM_BLOCK) k_dp_exit(const uint16_t* __restrict__ delta, uint32_t count, uint32_t T, uint32_t* __restrict__ X0) {
  extern __shared__ uint16_t dp_lds[];
  uint16_t *a = dp_lds, *b = dp_lds + T;
  const uint32_t t = blockIdx.x, start = t * T, Tt = count - start < T ? count - start : T;  // start < count by the grid
  for (uint32_t j = threadIdx.x; j < Tt; j += DM_BLOCK) a[j] = (uint16_t)(j + delta[start + j]);
  __syncthreads();
  for (uint32_t span = 1; span < Tt; span <<= 1) {  // after r rounds a[j] is 2^r jumps from j, or the exit
    for (uint32_t j = threadIdx.x; j < Tt; j += DM_BLOCK) { const uint32_t x = a[j]; b[j] = x < Tt ? a[x] : (uint16_t)x; }
    __syncthreads();
    uint16_t* s = a; a = b; b = s;
  }
  const uint32_t heads = Tt < DP_HEAD ? Tt : DP_HEAD;
  for (uint32_t j = threadIdx.x; j < heads; j += DM_BLOCK) X0[(size_t)t * DP_HEAD + j] = start + a[j];
}
// blockDim = DP_HEAD: lane h follows the group's position h out of the group
__global__ void __launch_bounds__(DP_HEAD) k_dp_compose(const uint32_t* __restrict__ X0, uint32_t count, uint32_t T, uint32_t G, uint32_t* __restrict__ X1) {
  const uint32_t g = blockIdx.x, h = threadIdx.x;
  const uint32_t gstart = g * G * T, gend_tile = (g + 1) * G;
  uint32_t pos = gstart + h;
  if (pos >= count) return;
  while (pos < count && pos / T < gend_tile) { const uint32_t t = pos / T; pos = X0[(size_t)t * DP_HEAD + (pos - t * T)]; }
  X1[(size_t)g * DP_HEAD + h] = pos;
}
// one lane: carry[0] the entry of this segment, carry[1] that of the next (written here only when the prologue already reaches the end)
__global__ void k_dp_top(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, const uint32_t* __restrict__ Ab,
                         const uint32_t* __restrict__ Bb, size_t first, uint32_t count, unsigned mp0, unsigned mp1, uint32_t* __restrict__ tok,
                         const uint32_t* __restrict__ X1, uint32_t T, uint32_t G, uint32_t* __restrict__ Eg, DpCarry* __restrict__ carry) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t pos = carry[0].entry;
  unsigned sl = carry[0].sl, sd = carry[0].sd, fb = 0;
  if (sl && pos < count) pos = dp_segment_walk<true>(D, n, Lw, Ab, Bb, first, count, pos, sl, sd, mp0, mp1, tok, fb);
  if (pos >= count) { carry[1].entry = pos - count; carry[1].sl = sl; carry[1].sd = sd; carry[1].fallbacks = carry[0].fallbacks + fb; return; }
  carry[1].fallbacks = carry[0].fallbacks + fb;  // the token kernel adds its own
  const uint32_t GT = G * T;
  while (pos < count) { const uint32_t g = pos / GT; Eg[g] = pos; pos = X1[(size_t)g * DP_HEAD + (pos - g * GT)]; }
}
__global__ void __launch_bounds__(64) k_dp_down(const uint32_t* __restrict__ X0, uint32_t count, uint32_t T, uint32_t G, uint32_t ngroups,
                                                const uint32_t* __restrict__ Eg, uint32_t* __restrict__ Et) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= ngroups) return;
  uint32_t pos = Eg[g];
  const uint32_t gend_tile = (g + 1) * G;
  while (pos < count && pos / T < gend_tile) { const uint32_t t = pos / T; Et[t] = pos; pos = X0[(size_t)t * DP_HEAD + (pos - t * T)]; }
}
__global__ void __launch_bounds__(64) k_dp_mark(uint16_t* __restrict__ delta, uint32_t count, uint32_t T, uint32_t ntiles, const uint32_t* __restrict__ Et) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= ntiles) return;
  uint32_t pos = Et[t];
  const uint32_t end = (t + 1) * T < count ? (t + 1) * T : count;
  while (pos < end) { const uint32_t d = delta[pos]; delta[pos] = (uint16_t)(d | DP_MARK); pos += d; }
}
__global__ void __launch_bounds__(DM_BLOCK) k_dp_tokens(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lw, const uint32_t* __restrict__ Ab,
                                                        const uint32_t* __restrict__ Bb, size_t first, uint32_t count, unsigned mp0, unsigned mp1,
                                                        const uint16_t* __restrict__ delta, uint32_t* __restrict__ tok, DpCarry* __restrict__ carry) {
  const uint32_t i = blockIdx.x * DM_BLOCK + threadIdx.x;
  if (i >= count || !(delta[i] & DP_MARK)) return;
  unsigned sl = 0, sd = 0, fb = 0;
  const uint32_t next = dp_segment_walk<true>(D, n, Lw, Ab, Bb, first, count, i, sl, sd, mp0, mp1, tok, fb);
  if (fb) atomicAdd(&carry[1].fallbacks, fb);
  if (next >= count) { carry[1].entry = next - count; carry[1].sl = sl; carry[1].sd = sd; }  // the one reachable walk that ends the segment
}
struct DpNonZero {
  __device__ bool operator()(const uint32_t& t) const { return t != 0; }
};

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
  hipEvent_t ev[2][7] = {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
  // the parse (sp_deflate_open_parse): per position of one segment 2 bytes of jumps, 4 of token words, 1536 / T of exits; the host gets tokens
  bool parse = false;
  uint32_t T = 0, G = 0;
  uint16_t* delta = nullptr;
  uint32_t *tok = nullptr, *X0 = nullptr, *X1 = nullptr, *Eg = nullptr, *Et = nullptr;
  DpCarry* carry = nullptr;  // [nseg + 1]: carry[s] is segment s's entry
  void* sel_tmp = nullptr;
  size_t sel_bytes = 0;
  // the coder on the device too (sp_deflate_open_emit; deflate_emit.hip): the compacted tokens stay in its lists, the host gets block records
  bool coded = false;
  size_t chunk = 0;
  DeEmit* emit = nullptr;
  size_t ntiles_of(size_t count) const { return (count + T - 1) / T; }
  size_t ngroups_of(size_t count) const { return (count + (size_t)T * G - 1) / ((size_t)T * G); }
  size_t first_of(size_t s) const { return s * seg; }
  size_t count_of(size_t s) const { return n - s * seg < seg ? n - s * seg : seg; }
  // byte offsets into a pinned slot, set once at open. A and the tokens stand at 0.
  //   tables  [A: 4 seg][B: 4 seg][L: 2 seg][bytes: seg + DM_AHEAD]
  //   parse   [tokens: 4 (seg + 1), padded to 8][their number: 8][the next segment's entry: 16][bytes: seg + DM_AHEAD]
  //   coded   [the next segment's entry: 16]: tokens and bytes stay on the device, the records come down through the coder's own slots
  struct Slot { size_t B = 0, L = 0, N = 0, C = 0, D = 0, bytes = 0; } slot;
  void lay_out_slot() {
    if (coded) { slot.D = sizeof(DpCarry); slot.bytes = slot.D; return; }
    if (parse) { slot.N = (4 * (seg + 1) + 7) / 8 * 8; slot.C = slot.N + 8; slot.D = slot.C + sizeof(DpCarry); }
    else { slot.B = 4 * seg; slot.L = 8 * seg; slot.D = 10 * seg; }
    slot.bytes = slot.D + seg + DM_AHEAD;
  }
  template <typename T_> T_* at(int k, size_t off) const { return (T_*)(pin[k] + off); }
};

extern "C" {
void sp_deflate_close(sp_deflate* d) {
  if (!d) return;
  (void)hipSetDevice(d->ctx->dev);
  if (d->st) (void)hipStreamSynchronize(d->st);
  de_close(d->emit);
  for (auto& slot : d->ev)
    for (hipEvent_t e : slot)
      if (e) (void)hipEventDestroy(e);
  for (uint8_t* p : d->pin)
    if (p) (void)hipHostFree(p);
  for (void* p : {(void*)d->dD_own, (void*)d->head, (void*)d->Lw, (void*)d->keys_in, (void*)d->keys_out, (void*)d->Ab, (void*)d->Bb, (void*)d->vals_in,
                  (void*)d->vals_out, d->tmp, (void*)d->delta, (void*)d->tok, (void*)d->X0, (void*)d->X1, (void*)d->Eg, (void*)d->Et, (void*)d->carry,
                  d->sel_tmp})
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
                                   tdefl::HBITS, d->st));
  HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_last, (const uint16_t*)nullptr, (uint16_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, last_m, 0u,
                                   tdefl::HBITS, d->st));
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
  if (d->parse) {
    const size_t tiles = d->ntiles_of(seg), groups = d->ngroups_of(seg);
    HIPCHK(rocprim::select(nullptr, d->sel_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t*)nullptr, seg + 1, DpNonZero(), d->st));
    HIPCHK(hipMalloc(&d->sel_tmp, d->sel_bytes ? d->sel_bytes : 256));
    HIPCHK(hipMalloc((void**)&d->delta, 2 * seg));
    HIPCHK(hipMalloc((void**)&d->tok, 4 * (seg + 1)));
    HIPCHK(hipMalloc((void**)&d->X0, 4 * (size_t)DP_HEAD * tiles));
    HIPCHK(hipMalloc((void**)&d->X1, 4 * (size_t)DP_HEAD * groups));
    HIPCHK(hipMalloc((void**)&d->Eg, 4 * groups));
    HIPCHK(hipMalloc((void**)&d->Et, 4 * tiles));
    HIPCHK(hipMalloc((void**)&d->carry, sizeof(DpCarry) * (d->nseg + 1)));
    HIPCHK(hipMemsetAsync(d->carry, 0, sizeof(DpCarry) * (d->nseg + 1), d->st));
    if (d->coded) SPCHK(de_open(&d->emit, d->st, d->dD, d->n, seg, d->nseg, d->chunk));
  }
  for (uint8_t*& p : d->pin) HIPCHK(hipHostMalloc((void**)&p, d->slot.bytes, hipHostMallocDefault));
  HIPCHK(hipMemsetAsync(d->head, 0, 2 * DM_DICT, d->st));
  HIPCHK(hipMemsetAsync(d->Lw, 0, 2 * DM_DICT, d->st));
  HIPCHK(hipMemsetAsync(d->Ab, 0, 4, d->st));
  return SP_OK;
}
static int32_t deflate_open_form(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, bool parse, size_t tile, size_t group,
                                 sp_deflate** out, bool coded = false, size_t chunk = 0) {
  if (!c || !out || (n && !data) || probes == 0 || probes > 0xFFF) return SP_EINVAL;
  if (!tile) tile = 1024;
  if (!group) group = 64;
  if (parse && (tile < 512 || tile > 4096 || group < 2 || group > 4096)) return SP_EINVAL;  // a tile holds a jump (384) and fits the exits' LDS
  if (coded && chunk && (chunk < 256 || chunk > 65536)) return SP_EINVAL;                    // a chunk is a workgroup's worth of tokens at least
  sp_deflate* d = new (std::nothrow) sp_deflate();
  if (!d) return SP_ENOMEM;
  d->ctx = c;
  d->n = n;
  d->parse = parse; d->coded = coded; d->chunk = chunk;
  d->T = (uint32_t)tile; d->G = (uint32_t)group;
  const size_t opt = (size_t)c->opt.v[OPT_DIGEST_SEGMENT];
  d->seg = n < opt ? (n < DM_DICT ? DM_DICT : n) : opt;  // a short input is one segment of its own length (never below the window)
  d->nseg = (n + d->seg - 1) / d->seg;
  d->lay_out_slot();
  tdefl::probe_budget(probes, d->mp);
  const int32_t rc = deflate_open(d, data, on_device);
  if (rc != SP_OK) { sp_deflate_close(d); d = nullptr; }
  *out = d;
  return rc;
}
int32_t sp_deflate_open(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, sp_deflate** out) {
  return deflate_open_form(c, data, n, on_device, probes, false, 0, 0, out);
}
int32_t sp_deflate_open_parse(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, size_t tile, size_t group, sp_deflate** out) {
  return deflate_open_form(c, data, n, on_device, probes, true, tile, group, out);
}
int32_t sp_deflate_open_emit(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, size_t tile, size_t group, size_t chunk,
                             sp_deflate** out) {
  return deflate_open_form(c, data, n, on_device, probes, true, tile, group, out, true, chunk);
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
    HIPCHK(rocprim::radix_sort_pairs(d->tmp, d->tmp_bytes, (const uint16_t*)d->keys_in, d->keys_out, (const uint32_t*)d->vals_in, d->vals_out, m, 0u, tdefl::HBITS, st));
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
  if (d->parse) {
    const uint32_t cnt = (uint32_t)count, T = d->T, G = d->G, tiles = (uint32_t)d->ntiles_of(count), groups = (uint32_t)d->ngroups_of(count);
    const uint16_t* Lw = d->Lw;
    const uint32_t *Ab = d->Ab, *Bb = d->Bb;
    DpCarry* carry = d->carry + s;
    HIPCHK(hipMemsetAsync(d->tok, 0, 4 * (count + 1), st));
    HIPCHK(hipMemsetAsync(d->Eg, 0xFF, 4 * (size_t)groups, st));
    HIPCHK(hipMemsetAsync(d->Et, 0xFF, 4 * (size_t)tiles, st));
    hipLaunchKernelGGL(k_dp_jump, dm_grid(count), dim3(DM_BLOCK), 0, st, d->dD, n, Lw, Ab, Bb, first, cnt, d->mp[0], d->mp[1], d->delta);
    hipLaunchKernelGGL(k_dp_exit, dim3(tiles), dim3(DM_BLOCK), 4 * (size_t)T, st, (const uint16_t*)d->delta, cnt, T, d->X0);
    hipLaunchKernelGGL(k_dp_compose, dim3(groups), dim3(DP_HEAD), 0, st, (const uint32_t*)d->X0, cnt, T, G, d->X1);
    hipLaunchKernelGGL(k_dp_top, dim3(1), dim3(64), 0, st, d->dD, n, Lw, Ab, Bb, first, cnt, d->mp[0], d->mp[1], d->tok, (const uint32_t*)d->X1, T, G, d->Eg, carry);
    hipLaunchKernelGGL(k_dp_down, dim3((groups + 63) / 64), dim3(64), 0, st, (const uint32_t*)d->X0, cnt, T, G, groups, (const uint32_t*)d->Eg, d->Et);
    hipLaunchKernelGGL(k_dp_mark, dim3((tiles + 63) / 64), dim3(64), 0, st, d->delta, cnt, T, tiles, (const uint32_t*)d->Et);
    HIPCHK(hipEventRecord(d->ev[k][5], st));
    hipLaunchKernelGGL(k_dp_tokens, dm_grid(count), dim3(DM_BLOCK), 0, st, d->dD, n, Lw, Ab, Bb, first, cnt, d->mp[0], d->mp[1], (const uint16_t*)d->delta, d->tok,
                       carry);
    if (hipGetLastError() != hipSuccess) return SP_EHIP;
    // the compaction writes the dense list and its length straight into the pinned slot, or into the device coder's list
    HIPCHK(rocprim::select(d->sel_tmp, d->sel_bytes, (const uint32_t*)d->tok, d->coded ? de_tokens(d->emit, s) : d->at<uint32_t>(k, 0),
                           d->coded ? de_ntok(d->emit, s) : d->at<size_t>(k, d->slot.N), count + 1, DpNonZero(), st));
    HIPCHK(hipEventRecord(d->ev[k][6], st));
    if (d->coded) SPCHK(de_segment_blocks(d->emit, s, first, count));
    HIPCHK(hipMemcpyAsync(d->at<DpCarry>(k, d->slot.C), carry + 1, sizeof(DpCarry), hipMemcpyDeviceToHost, st));
  } else {
    HIPCHK(hipMemcpyAsync(d->at<uint32_t>(k, 0), d->Ab + 1, 4 * count, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(d->at<uint32_t>(k, d->slot.B), d->Bb, 4 * count, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(d->at<uint16_t>(k, d->slot.L), Lseg, 2 * count, hipMemcpyDeviceToHost, st));
  }
  if (!d->coded) HIPCHK(hipMemcpyAsync(d->at<uint8_t>(k, d->slot.D), d->dD + first, nbytes, hipMemcpyDeviceToHost, st));
  if (s + 1 < d->nseg) {  // count == seg >= 32768 here: what the next segment needs of this one
    HIPCHK(hipMemcpyAsync(d->Ab, d->Ab + count, 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(d->Lw, d->Lw + count, 2 * DM_DICT, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipEventRecord(d->ev[k][4], st));
  d->started = s + 1;
  return SP_OK;
}

// segment s of a handle of the given form is ready in its pinned slot
static int32_t deflate_segment_ready(sp_deflate* d, bool parse, size_t s, size_t* first, size_t* count, bool coded = false) {
  if (!d || d->parse != parse || d->coded != coded || s >= d->started || s + 2 < d->started) return SP_EINVAL;
  HIPCHK(hipSetDevice(d->ctx->dev));
  HIPCHK(hipEventSynchronize(d->ev[s & 1][4]));
  if (first) *first = d->first_of(s);
  if (count) *count = d->count_of(s);
  return SP_OK;
}
// device time of the segment's stages, between the events in the order the form recorded them (event 4 is the last of both)
//   tables  links, search A, search B, copies
//   parse   links, search A, search B, reachability, tokens + compaction, copies (coded: the block stage and the records' copy)
static int32_t deflate_stage_ms(const sp_deflate* d, int k, double* ms) {
  static const int order[2][7] = {{0, 1, 2, 3, 4, -1, -1}, {0, 1, 2, 3, 5, 6, 4}};
  const int* o = order[d->parse];
  for (int i = 0; ms && o[i] != 4; i++) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, d->ev[k][o[i]], d->ev[k][o[i + 1]]));
    ms[i] = t;
  }
  return SP_OK;
}
int32_t sp_deflate_segment_wait(sp_deflate* d, size_t s, size_t* first, size_t* count, const uint8_t** bytes, const uint16_t** L, const uint32_t** A,
                                const uint32_t** B, double* ms) {
  SPCHK(deflate_segment_ready(d, false, s, first, count));
  const int k = (int)(s & 1);
  if (bytes) *bytes = d->at<uint8_t>(k, d->slot.D);
  if (L) *L = d->at<uint16_t>(k, d->slot.L);
  if (A) *A = d->at<uint32_t>(k, 0);
  if (B) *B = d->at<uint32_t>(k, d->slot.B);
  return deflate_stage_ms(d, k, ms);
}
int32_t sp_deflate_segment_wait_tokens(sp_deflate* d, size_t s, size_t* first, size_t* count, const uint8_t** bytes, const uint32_t** tokens, size_t* ntok,
                                       uint64_t* carry, double* ms) {
  SPCHK(deflate_segment_ready(d, true, s, first, count));
  const int k = (int)(s & 1);
  if (bytes) *bytes = d->at<uint8_t>(k, d->slot.D);
  if (tokens) *tokens = d->at<uint32_t>(k, 0);
  if (ntok) *ntok = *d->at<size_t>(k, d->slot.N);
  if (carry) {
    const DpCarry* c = d->at<DpCarry>(k, d->slot.C);
    carry[0] = d->first_of(s) + d->count_of(s) + c->entry; carry[1] = c->sl; carry[2] = c->sd; carry[3] = c->fallbacks;
  }
  return deflate_stage_ms(d, k, ms);
}

int32_t sp_deflate_segment_wait_blocks(sp_deflate* d, size_t s, size_t* first, size_t* count, size_t* nblocks, const uint64_t** records,
                                       const uint16_t** hist, uint64_t* adler, uint64_t* carry, double* ms) {
  SPCHK(deflate_segment_ready(d, true, s, first, count, true));
  const int k = (int)(s & 1);
  SPCHK(de_blocks(d->emit, s, nblocks, records, hist, adler));
  if (carry) {
    const DpCarry* c = d->at<DpCarry>(k, d->slot.C);
    carry[0] = d->first_of(s) + d->count_of(s) + c->entry; carry[1] = c->sl; carry[2] = c->sd; carry[3] = c->fallbacks;
  }
  return deflate_stage_ms(d, k, ms);
}
int32_t sp_deflate_segment_emit(sp_deflate* d, size_t s, size_t nblocks, const uint64_t* plans, const uint32_t* tables, const uint8_t* headers) {
  if (!d || !d->coded || s >= d->started || s + 2 < d->started) return SP_EINVAL;
  HIPCHK(hipSetDevice(d->ctx->dev));
  return de_segment_emit(d->emit, s, nblocks, plans, tables, headers);
}
int32_t sp_deflate_emit_bytes(sp_deflate* d, uint8_t* out, size_t nbytes, double* ms) {
  if (!d || !d->coded) return SP_EINVAL;
  if (!d->emit) return nbytes ? SP_EINVAL : SP_OK;  // an empty input has no segment and no bytes here
  HIPCHK(hipSetDevice(d->ctx->dev));
  return de_bytes(d->emit, out, nbytes, ms);
}
}  // extern "C"

// the whole input through an opened handle, one segment after the other: each(s) waits for segment s and takes what it wants; closes the handle
template <typename Each>
static int32_t deflate_whole(sp_deflate* d, Each each) {
  int32_t rc = SP_OK;
  for (size_t s = 0; s < d->nseg && rc == SP_OK; s++) {
    rc = sp_deflate_segment_start(d, s);
    if (rc == SP_OK) rc = each(s);
  }
  sp_deflate_close(d);
  return rc;
}

extern "C" {
int32_t sp_deflate_tokens(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, size_t tile, size_t group, uint32_t* tokens,
                          size_t* ntok, uint64_t* info) {
  if (!ntok) return SP_EINVAL;
  sp_deflate* d = nullptr;
  SPCHK(sp_deflate_open_parse(c, data, n, on_device, probes, tile, group, &d));
  const size_t nseg = d->nseg;
  size_t total = 0;
  uint64_t held = 0, fallbacks = 0;
  const int32_t rc = deflate_whole(d, [&](size_t s) -> int32_t {
    const uint32_t* t;
    size_t cnt = 0;
    uint64_t carry[4];
    SPCHK(sp_deflate_segment_wait_tokens(d, s, nullptr, nullptr, nullptr, &t, &cnt, carry, nullptr));
    if (total + cnt > n) return SP_EINVAL;  // more tokens than positions: never, and never written past the caller's array
    if (tokens) memcpy(tokens + total, t, 4 * cnt);
    total += cnt;
    if (carry[1] && s + 1 < nseg) held++;
    fallbacks = carry[3];
    return SP_OK;
  });
  *ntok = total;
  if (info) { info[0] = held; info[1] = fallbacks; }
  return rc;
}
int32_t sp_deflate_blocks(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, size_t tile, size_t group, uint64_t* records,
                          uint16_t* hist, size_t cap, size_t* nblocks) {
  if (!nblocks || !records || !hist) return SP_EINVAL;
  if (!n) {  // no segment: the one block is the empty finish block
    if (!c || !cap) return SP_EINVAL;
    memset(records, 0, 8 * DE_REC_WORDS);
    memset(hist, 0, 2 * DE_HIST);
    records[3] = tdefl::RULE_FINISH;
    *nblocks = 1;
    return SP_OK;
  }
  sp_deflate* d = nullptr;
  SPCHK(sp_deflate_open_emit(c, data, n, on_device, probes, tile, group, 0, &d));
  size_t total = 0;
  const int32_t rc = deflate_whole(d, [&](size_t s) -> int32_t {
    size_t nb = 0;
    const uint64_t* r;
    const uint16_t* h;
    SPCHK(sp_deflate_segment_wait_blocks(d, s, nullptr, nullptr, &nb, &r, &h, nullptr, nullptr, nullptr));
    if (total + nb > cap) return SP_EINVAL;
    memcpy(records + DE_REC_WORDS * total, r, 8 * DE_REC_WORDS * nb);
    memcpy(hist + DE_HIST * total, h, 2 * DE_HIST * nb);
    total += nb;
    return SP_OK;
  });
  *nblocks = total;
  return rc;
}
int32_t sp_deflate_matches(sp_ctx* c, const uint8_t* data, size_t n, int on_device, uint32_t probes, uint16_t* L, uint32_t* A, uint32_t* B) {
  sp_deflate* d = nullptr;
  SPCHK(sp_deflate_open(c, data, n, on_device, probes, &d));
  return deflate_whole(d, [&](size_t s) -> int32_t {
    size_t first = 0, count = 0;
    const uint16_t* l; const uint32_t *a, *b;
    SPCHK(sp_deflate_segment_wait(d, s, &first, &count, nullptr, &l, &a, &b, nullptr));
    if (L) memcpy(L + first, l, 2 * count);
    if (A) memcpy(A + first, a, 4 * count);
    if (B) memcpy(B + first, b, 4 * count);
    return SP_OK;
  });
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
