// spartan_amd: the rules of miniz's tdefl (lazy parsing, levels 4..10) that the host's restatements (host/deflate.cc) and the device's search
// and parse (deflate_match.hip) both run, written once. Stateless and SP_HD, as field.hpp is. host/deflate.cc's sequential deflater (Tdefl::run,
// Tdefl::find_match) is the form pinned against the real miniz and the oracle of everything here: it shares nothing with this file on purpose.
//
// The search as one independent item per input position. tdefl's find_match reads three things that depend on how far the parser has come:
// the ring `dict`, the ring `next`, and dict_size. With the whole input D[0, n) in hand all three are functions of the position p alone:
//   lookahead   la = min(258, n - p);  dict_size = min(p, 32768 - la)
//   dict        dict[(q & 32767) + k] is D[q + k] for every q the search can reach (q >= p - dict_size: q + 32768 has not arrived yet)
//   next        the slot of such a q still holds q's own link L[q] = low 16 bits of the greatest q' < q with the same 3-byte hash (0: none).
//               The look-back is unbounded: a head written more than 65535 positions ago aliases, and tdefl follows the alias.
// find(p, init) is find_match with those substitutions and nothing else changed: probe budget, three-hop inner loop, c0/c1 filter, the
// dist == 0 break and the early return at the longest match. A table entry is dist | len << 16, (0, init) when nothing was found.
//
// The parse as walks between free states. The parser's state before a step is (q, held len, held dist); call it FREE when it holds no
// match. From a free state at p the look-up at p, filtered, is nothing (a literal at p, free at p + 1), a match of >= 128 (taken at once, free
// at p + len), or a match that is HELD. A held match found at q - 1 meets the look-up at q with init = its length: a longer one makes D[q - 1] a
// literal and is itself taken (>= 128) or held in turn; otherwise the held match is emitted at q - 1 and the state is free at q - 1 + len.
// Held lengths strictly grow from >= 3 and stay below 128, so a walk holds at most 125 times (positions p .. p + 124), its last step is at
// q <= p + 125 and the next free state F(p) is at most q + 258: 1 <= F(p) - p <= 383. Every token of a walk starts at a position of its own
// (a literal at each chain position that lost, the match at the last), so the parse is one word per input position.
//
// The token word: one per literal or match, in stream order. A literal carries its byte in bits 0..7 and length 0; a match (len, dist)
// carries dist - 1 in bits 0..14 and len in bits 15..23. Nothing in a walk reads the coder's state; the coder needs of a token only what
// the block check after the parser's STEP reads (lookahead_pos, dict_size), which two bits carry: TOK_CHECK (a check follows this token: a
// literal emitted together with a match of >= 128 has none, and a step that only holds emits nothing: its check sees the numbers of the check
// before it, which did not fire or reset them) and TOK_HELD (a match is held when that check runs: lookahead_pos is then one past the
// emitted bytes). TOK_VALID is always set, so that 0 is "no token starts here" in the device's one-word-per-position form.
#pragma once
#include "field.hpp"  // SP_HD

namespace tdefl {
constexpr unsigned DICT = 32768, DMASK = DICT - 1, MINM = 3, MAXM = 258, HBITS = 15;
constexpr unsigned FAR3 = 8192;  // a match of MINM at this distance or further is dropped
constexpr unsigned TAKE = 128;   // a match of this length is taken at once, never held
constexpr uint32_t TOK_VALID = 1u << 31, TOK_CHECK = 1u << 30, TOK_HELD = 1u << 29;

SP_HD unsigned hash3(const uint8_t* s) { return (((unsigned)s[0] << 10) ^ ((unsigned)s[1] << 5) ^ (unsigned)s[2]) & (DICT - 1); }
// hash-chain probes of a search from the flags' probe count: mp[0]; mp[1] once a match of >= 32 is in hand
SP_HD void probe_budget(unsigned probes, unsigned mp[2]) {
  mp[0] = 1 + ((probes & 0xFFF) + 2) / 3;
  mp[1] = 1 + (((probes & 0xFFF) >> 2) + 2) / 3;
}
SP_HD uint32_t pack(unsigned dist, unsigned len) { return dist | (len << 16); }
// what the parser keeps of the search's answer at `pos`: 0 (nothing) or the match
SP_HD uint32_t filter(uint32_t got, size_t pos) {
  const unsigned dist = got & 0xFFFFu, len = got >> 16;
  return !dist || (len == MINM && dist >= FAR3) || (unsigned)(pos & DMASK) == dist ? 0u : got;
}
// does A[pos] = a leave the filter as a HELD match (then the parser asks at pos + 1 with init = its length: table B)
SP_HD bool held(uint32_t a, size_t pos) { return filter(a, pos) && (a >> 16) < TAKE; }

SP_HD uint32_t tok_lit(unsigned c, uint32_t bits) { return TOK_VALID | bits | c; }
SP_HD uint32_t tok_match(unsigned len, unsigned dist, uint32_t bits) { return TOK_VALID | bits | (len << 15) | (dist - 1); }
SP_HD unsigned tok_len(uint32_t t) { return (t >> 15) & 0x1FF; }  // 0: a literal
SP_HD unsigned tok_dist(uint32_t t) { return (t & 0x7FFF) + 1; }

SP_HD uint32_t ld32(const uint8_t* p) {  // any alignment
  uint32_t x;
  __builtin_memcpy(&x, p, 4);
  return x;
}
// Lbase[q - Lfirst] = L[q] (index arithmetic modulo 2^64: Lfirst may lie "before" position 0); the caller keeps [p - 32768, p] addressable.
// Every index is bounded: D[p + k], k < la <= n - p; D[cand + k], cand < p; links of cand >= p - max_dist only.
SP_HD uint32_t find(const uint8_t* __restrict__ D, size_t n, const uint16_t* __restrict__ Lbase, size_t Lfirst, size_t p, unsigned init, const unsigned mp[2]) {
  const size_t left = n - p;
  const unsigned la = left < MAXM ? (unsigned)left : MAXM;
  const unsigned max_dist = p < (size_t)(DICT - la) ? (unsigned)p : DICT - la;
  unsigned dist = 0, best = 0, match_len = init;
  if (la <= match_len) return pack(0, init);
  unsigned probes_left = match_len >= 32 ? mp[1] : mp[0];
  const uint8_t* s = D + p;
  uint8_t c0 = s[match_len], c1 = s[match_len - 1];
  size_t cand = p;
  for (;;) {
    for (;;) {
      if (--probes_left == 0) return pack(best, match_len);
      bool hit = false;
#pragma unroll 1
      for (int k = 0; k < 3 && !hit; k++) {
        const unsigned nx = Lbase[cand - Lfirst];
        if (!nx || (dist = (((unsigned)p - nx) & 0xFFFFu)) > max_dist) return pack(best, match_len);
        cand = p - dist;
        if (D[cand + match_len] == c0 && D[cand + match_len - 1] == c1) hit = true;
      }
      if (hit) break;
    }
    if (!dist) break;
    const uint8_t* q = D + cand;
    unsigned probe_len = 0;
    bool differ = false;
    while (probe_len + 4 <= la) {  // four bytes a compare; the first differing byte is the lowest set one (little-endian on both sides)
      const uint32_t x = ld32(s + probe_len) ^ ld32(q + probe_len);
      if (x) { probe_len += (unsigned)__builtin_ctz(x) >> 3; differ = true; break; }
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
  return pack(best, match_len);
}

struct WalkState { size_t q; unsigned sl, sd; };  // next step at q; held match (sl, sd) found at q - 1, sl == 0: free
// The parser's steps from `w` until the state is free again (after at least one step) or q reaches `end`, where the parser's segment loop
// stops too (q passes `end` when a match crosses it). lookup(q, init) -> dist | len << 16;  emit(position the token starts at, token)
template <typename Lookup, typename Emit>
SP_HD void walk(const uint8_t* __restrict__ D, WalkState& w, size_t end, Lookup&& lookup, Emit&& emit) {
  do {
    const size_t q = w.q;
    const uint32_t got = filter(lookup(q, w.sl ? w.sl : MINM - 1), q);
    const unsigned cd = got & 0xFFFFu, cl = got >> 16;
    if (w.sl) {
      if (cl > w.sl) {
        if (cl >= TAKE) { emit(q - 1, tok_lit(D[q - 1], 0)); emit(q, tok_match(cl, cd, TOK_CHECK)); w.sl = 0; w.q = q + cl; }
        else { emit(q - 1, tok_lit(D[q - 1], TOK_CHECK | TOK_HELD)); w.sl = cl; w.sd = cd; w.q = q + 1; }
      } else {
        emit(q - 1, tok_match(w.sl, w.sd, TOK_CHECK));
        w.q = q - 1 + w.sl; w.sl = 0;
      }
    } else if (!got) {
      emit(q, tok_lit(D[q], TOK_CHECK)); w.q = q + 1;
    } else if (cl >= TAKE) {
      emit(q, tok_match(cl, cd, TOK_CHECK)); w.q = q + cl;
    } else {
      w.sl = cl; w.sd = cd; w.q = q + 1;
    }
  } while (w.sl && w.q < end);
}

// ---- the coder's rules: what a token costs, what it codes to, and when a block ends. tdefl's LZ code buffer holds a flag byte for every
// eight tokens (the first opened with the block), one byte a literal and three a match; the block check after a TOK_CHECK token reads the
// buffer's fill and the input bytes of the block so far, and the stored-block test at a check reads lookahead_pos and dict_size of the
// parser's step that the token closes.
constexpr unsigned LZBUF = 64 * 1024;
constexpr unsigned BLOCK_TOKENS = 58249;  // the most tokens of a block: literals until 1 + k + k / 8 > 65528 (k = 58248), and one unchecked literal more
enum BlockRule : uint32_t { RULE_NONE = 0, RULE_FULL = 1, RULE_RATIO = 2, RULE_FINISH = 3 };
SP_HD unsigned tok_code_bytes(uint32_t t) { return tok_len(t) ? 3u : 1u; }
SP_HD unsigned tok_input_bytes(uint32_t t) { const unsigned l = tok_len(t); return l ? l : 1u; }
// the code buffer's fill after k tokens of a block whose tok_code_bytes sum to `sum`
SP_HD uint64_t code_bytes_after(uint64_t sum, uint64_t k) { return 1 + sum + k / 8; }
SP_HD BlockRule block_check(uint64_t code_bytes, uint64_t total_lz_bytes) {
  if (code_bytes > LZBUF - 8) return RULE_FULL;
  if (total_lz_bytes > 31 * 1024 && ((code_bytes * 115) >> 7) >= total_lz_bytes) return RULE_RATIO;
  return RULE_NONE;
}
// lookahead_pos and dict_size after the parser's step that token t, which starts at input position pos, closes: a literal's step looked at
// pos (at pos + 1 when a match is held) and moved 1; a match taken at once looked at pos and moved len; a held match was found at pos, its
// step looked at pos + 1 and moved len - 1. The step at q with lookahead la = min(258, n - q) starts from dict_size = min(q, 32768 - la).
SP_HD void tok_step(uint32_t t, uint64_t pos, uint64_t n, uint64_t* lookahead_pos, uint32_t* dict_size) {
  const unsigned len = tok_len(t);
  uint64_t step, move;
  if (!len) { step = pos + ((t & TOK_HELD) ? 1 : 0); move = 1; }
  else if (len >= TAKE) { step = pos; move = len; }
  else { step = pos + 1; move = len - 1; }
  const uint64_t left = n - step, la = left < MAXM ? left : MAXM;
  const uint64_t ds = (step < DICT - la ? step : DICT - la) + move;
  *lookahead_pos = step + move;
  *dict_size = (uint32_t)(ds < DICT ? ds : DICT);
}
// RFC 1951's symbols in tdefl's indexing: a length 3..258 -> symbol 257..285, a distance 1..32768 -> symbol 0..29, each with the number of
// extra bits and their value
SP_HD void len_symbol(unsigned len, unsigned* sym, unsigned* nextra, unsigned* extra) {
  const unsigned l = len - MINM;
  if (l < 8) { *sym = 257 + l; *nextra = 0; *extra = 0; return; }
  if (len == MAXM) { *sym = 285; *nextra = 0; *extra = 0; return; }
  const unsigned e = (31 - (unsigned)__builtin_clz(l)) - 2;
  *sym = 257 + 4 * e + 4 + ((l >> e) & 3); *nextra = e; *extra = l & ((1u << e) - 1);
}
SP_HD void dist_symbol(unsigned dist, unsigned* sym, unsigned* nextra, unsigned* extra) {
  const unsigned d = dist - 1;
  if (d < 4) { *sym = d; *nextra = 0; *extra = 0; return; }
  const unsigned e = (31 - (unsigned)__builtin_clz(d)) - 1;
  *sym = 2 * (e + 1) + ((d >> e) & 1); *nextra = e; *extra = d & ((1u << e) - 1);
}
// A block's code tables as 320 words, code | size << 16: 288 of the literal/length alphabet, then 32 of the distances. The bits of a token
// under them, first bit lowest, at most 48 (15 + 5 + 15 + 13); returns their number.
constexpr unsigned TABLE_WORDS = 288 + 32;
SP_HD unsigned tok_bits(uint32_t t, const uint32_t* table, uint64_t* bits) {
  const unsigned len = tok_len(t);
  if (!len) { const uint32_t w = table[t & 0xFF]; *bits = w & 0xFFFF; return w >> 16; }
  unsigned s, ne, ev;
  len_symbol(len, &s, &ne, &ev);
  uint32_t w = table[s];
  uint64_t v = w & 0xFFFF;
  unsigned nb = w >> 16;
  v |= (uint64_t)ev << nb; nb += ne;
  dist_symbol(tok_dist(t), &s, &ne, &ev);
  w = table[288 + s];
  v |= (uint64_t)(w & 0xFFFF) << nb; nb += w >> 16;
  v |= (uint64_t)ev << nb; nb += ne;
  *bits = v;
  return nb;
}
// the same token's length in bits from the code sizes alone
SP_HD unsigned tok_nbits(uint32_t t, const uint32_t* table) {
  const unsigned len = tok_len(t);
  if (!len) return table[t & 0xFF] >> 16;
  unsigned s, ne, ev, nb;
  len_symbol(len, &s, &ne, &ev);
  nb = (table[s] >> 16) + ne;
  dist_symbol(tok_dist(t), &s, &ne, &ev);
  return nb + (table[288 + s] >> 16) + ne;
}
}  // namespace tdefl
