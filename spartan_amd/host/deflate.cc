// spartan_amd host driver: the zlib stream of R1CSShape::get_digest (src/r1cs.rs:154-158).
//
// The reference binds a NIZK proof to its instance by absorbing `digest = ZlibEncoder(Compression::default())(bincode(shape))` into
// the transcript (src/lib.rs:514): the digest is the COMPRESSED STREAM ITSELF, so byte parity needs the exact deflater.
// flate2 = "1.0.14" with the rust_backend (Cargo.toml:31,75) is miniz_oxide, a line-by-line port of miniz's tdefl; neither is under
// /root/reference. This file restates tdefl's level-6 path (what Compression::default() selects) from the published algorithm:
//   * parameters (tdefl_create_comp_flags_from_zip_params(6, 15, 0)): 128 hash-chain probes (43 once a match of >= 32 is held),
//     lazy parsing (greedy only up to level 3), zlib header, Adler-32 trailer;
//   * dictionary 32 KiB, 3-byte hash (b0 << 10 ^ b1 << 5 ^ b2) & 32767 with 16-bit position chains, matches 3..258, a length-3 match
//     further than 8 KiB away is dropped, a held match of >= 128 is taken at once;
//   * a block ends when the 64 KiB LZ code buffer is nearly full or, past 31 KiB of input, when the code buffer stops paying
//     (code bytes * 115 / 128 >= input bytes); each block is dynamic-Huffman (static below 48 input bytes), or stored when the
//     coded form is not smaller; code lengths by the in-place minimum-redundancy algorithm over the frequency-sorted symbols
//     (stable: ties by symbol index), limited to 15 / 7 bits by the Kraft fix-up, code-length alphabet run-length packed as tdefl does.
// PINNED AGAINST THE REAL C MINIZ (tests/test_host_transcript.py::test_deflater_equals_real_miniz): libtorch_cpu.so in this image bundles
// miniz 3.0.2 and exports mz_compress2; at every lazy-parsing level (4..10, i.e. 16/32/128/256/512/768/1500 probes — level 6 is what
// flate2's Compression::default() selects) the WHOLE zlib stream of this file, header and Adler-32 included, equals miniz's on the bincode
// of synthetic R1CS shapes 2^4..2^16 (multi-block, dynamic Huffman), random data (stored blocks), text, and block-boundary inputs. The
// stream also inflates (Python zlib) to exactly the bincode the oracle serialises. What stays unpinned is only that miniz_oxide (a
// line-by-line Rust port of tdefl) equals miniz; scripts/compare_with_libspartan.sh prints both digests. The header bytes are the one
// documented variable: miniz >= 2.2 and miniz_oxide >= 0.4 derive FLEVEL from the probe count (level 6: 0x78 0x9C), older ones write
// 0x78 0x01 (the `old_header` argument — an explicit API parameter, spz_instance_set_digest_header, never an environment switch).
// Below the sequential deflater (Tdefl::run and Tdefl::find_match: the oracle of everything that follows, left as it was and sharing
// nothing with it) stand the restatements that run behind the device. Their rules — the search as one independent item per input position
// (find), the parser's step as walks between FREE states (walk), the candidate filter, the token word — are csrc/tdefl_rules.hpp, which
// csrc/deflate_match.hip runs on the device; here they are applied on the host:
//   deflate_links_host, deflate_matches_host   the tables L, A, B over a whole input
//   TableLookup                                the parser's look-up answered from such tables: A, or B, or a search on the spot
//   Coder                                      record_literal, record_match, the block check and flush_block (the Tdefl members, untouched)
//                                              fed one token at a time, with Adler-32 as the input arrives: no tables, no search
//   MatchParser, zlib_from_matches             TableLookup -> walk -> Coder, segment by segment: what digest.cc runs behind the device search
//   deflate_tokens_host                        TableLookup -> walk -> a token list: the host model of the device parse
//   TokenCoder, zlib_from_tokens               a token list -> Coder: what digest.cc runs behind the device parse
//   deflate_blocks_host                        a token list -> block records and histograms, from prefix sums of token costs: the host model
//                                              of the device coder's block stage (csrc/deflate_emit.hip)
//   BlockPlanner                               a block's record and histogram -> its tables, header, stored-or-coded decision and bit offset
//                                              (optimize_table, start_dynamic_block, start_static_block of Tdefl, untouched): what digest.cc
//                                              runs behind the device coder
//   zlib_from_blocks                           records -> BlockPlanner -> every token's bits ORed in at its own offset: the host model of the
//                                              device's emission
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "libspartan.hpp"  // MatchParser and the declarations of what this file defines

namespace spz {
namespace {
constexpr unsigned DICT = 32768, DMASK = DICT - 1, MINM = 3, MAXM = 258, LZBUF = 64 * 1024, HBITS = 15, HSHIFT = 5, HSIZE = 1u << HBITS;

struct SymFreq { uint16_t key, sym; };

struct Tdefl {
  std::vector<uint8_t> out;
  uint64_t bitbuf = 0;
  unsigned bits_in = 0;
  uint8_t dict[DICT + MAXM - 1];
  uint16_t next[DICT], hash[HSIZE];
  // LZ codes of the current block: tokens + the byte count tdefl's code buffer would hold (flag bytes included)
  struct Tok { uint16_t len_m3, dist_m1; bool match; uint8_t lit; };
  std::vector<Tok> toks;
  size_t code_bytes = 1;       // pLZ_code_buf - lz_code_buf (starts past the first flag byte)
  unsigned flags_left = 8;
  uint16_t count[3][288];
  uint16_t codes[3][288];
  uint8_t sizes[3][288];
  unsigned lookahead_pos = 0, lookahead_size = 0, dict_size = 0, total_lz_bytes = 0, lz_dict_pos = 0, block_index = 0;
  unsigned saved_match_dist = 0, saved_match_len = 0, saved_lit = 0;
  unsigned max_probes[2];
  uint32_t adler = 1;
  bool old_header = false;
  unsigned probes = 128;  // tdefl flags & 0xFFF: s_tdefl_num_probes[level] = {0, 1, 6, 32, 16, 32, 128, 256, 512, 768, 1500}; 128 = level 6
  // the table-driven parser (MatchParser below) keeps no dictionary: the bytes of a stored block then come from the input itself
  const uint8_t* stored_src = nullptr;
  size_t stored_pos = 0;  // lz_dict_pos without the 32-bit wrap: where the current block began in stored_src
  unsigned static_blocks = 0, stored_blocks = 0;  // counted for the token coder's tests; nothing reads them here

  void put(unsigned b, unsigned l) {
    bitbuf |= (uint64_t)b << bits_in;
    bits_in += l;
    while (bits_in >= 8) { out.push_back((uint8_t)bitbuf); bitbuf >>= 8; bits_in -= 8; }
  }
  // ---- symbol tables of RFC 1951 in tdefl's indexing: length - 3 -> (symbol, extra bits); distance - 1 -> (symbol, extra bits)
  static void len_code(unsigned len_m3, unsigned* sym, unsigned* nextra) {
    static const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    unsigned len = len_m3 + 3, k = 28;
    while (base[k] > len) k--;
    *sym = 257 + k; *nextra = extra[k];
  }
  static void dist_code(unsigned dist_m1, unsigned* sym, unsigned* nextra) {
    static const uint16_t base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    unsigned dist = dist_m1 + 1, k = 29;
    while (base[k] > dist) k--;
    *sym = k; *nextra = extra[k];
  }

  void record_literal(uint8_t lit) {
    total_lz_bytes++;
    toks.push_back(Tok{0, 0, false, lit});
    code_bytes += 1;
    if (--flags_left == 0) { flags_left = 8; code_bytes++; }
    count[0][lit]++;
  }
  void record_match(unsigned len, unsigned dist) {
    total_lz_bytes += len;
    toks.push_back(Tok{(uint16_t)(len - MINM), (uint16_t)(dist - 1), true, 0});
    code_bytes += 3;
    if (--flags_left == 0) { flags_left = 8; code_bytes++; }
    unsigned s, e;
    dist_code(dist - 1, &s, &e);
    count[1][s]++;
    len_code(len - MINM, &s, &e);
    count[0][s]++;
  }

  // ---- Huffman tables (tdefl_optimize_huffman_table)
  static void minimum_redundancy(SymFreq* A, int n) {  // in-place: keys become code lengths (frequency-sorted input)
    int root, leaf, next, avbl, used, dpth;
    if (n == 0) return;
    if (n == 1) { A[0].key = 1; return; }
    A[0].key = (uint16_t)(A[0].key + A[1].key); root = 0; leaf = 2;
    for (next = 1; next < n - 1; next++) {
      if (leaf >= n || A[root].key < A[leaf].key) { A[next].key = A[root].key; A[root++].key = (uint16_t)next; } else A[next].key = A[leaf++].key;
      if (leaf >= n || (root < next && A[root].key < A[leaf].key)) { A[next].key = (uint16_t)(A[next].key + A[root].key); A[root++].key = (uint16_t)next; }
      else A[next].key = (uint16_t)(A[next].key + A[leaf++].key);
    }
    A[n - 2].key = 0;
    for (next = n - 3; next >= 0; next--) A[next].key = (uint16_t)(A[A[next].key].key + 1);
    avbl = 1; used = dpth = 0; root = n - 2; next = n - 1;
    while (avbl > 0) {
      while (root >= 0 && (int)A[root].key == dpth) { used++; root--; }
      while (avbl > used) { A[next--].key = (uint16_t)dpth; avbl--; }
      avbl = 2 * used; dpth++; used = 0;
    }
  }
  static void enforce_max_code_size(int* num_codes, int code_list_len, int max_code_size) {
    if (code_list_len <= 1) return;
    for (int i = max_code_size + 1; i <= 32; i++) num_codes[max_code_size] += num_codes[i];
    uint32_t total = 0;
    for (int i = max_code_size; i > 0; i--) total += ((uint32_t)num_codes[i]) << (max_code_size - i);
    while (total != (1u << max_code_size)) {
      num_codes[max_code_size]--;
      for (int i = max_code_size - 1; i > 0; i--)
        if (num_codes[i]) { num_codes[i]--; num_codes[i + 1] += 2; break; }
      total--;
    }
  }
  void optimize_table(int t, int table_len, int limit, bool is_static) {
    int num_codes[1 + 32];
    unsigned next_code[32 + 1];
    memset(num_codes, 0, sizeof num_codes);
    if (is_static) {
      for (int i = 0; i < table_len; i++) num_codes[sizes[t][i]]++;
    } else {
      SymFreq syms[288];
      int n = 0;
      for (int i = 0; i < table_len; i++)
        if (count[t][i]) { syms[n].key = count[t][i]; syms[n++].sym = (uint16_t)i; }
      std::stable_sort(syms, syms + n, [](const SymFreq& a, const SymFreq& b) { return a.key < b.key; });  // tdefl's two-pass LSD radix sort
      minimum_redundancy(syms, n);
      for (int i = 0; i < n; i++) num_codes[syms[i].key]++;
      enforce_max_code_size(num_codes, n, limit);
      memset(sizes[t], 0, sizeof sizes[t]);
      memset(codes[t], 0, sizeof codes[t]);
      for (int i = 1, j = n; i <= limit; i++)
        for (int l = num_codes[i]; l > 0; l--) sizes[t][syms[--j].sym] = (uint8_t)i;
    }
    next_code[1] = 0;
    for (int j = 0, i = 2; i <= limit; i++) next_code[i] = j = ((j + num_codes[i - 1]) << 1);
    for (int i = 0; i < table_len; i++) {
      unsigned rev = 0, code, sz = sizes[t][i];
      if (!sz) continue;
      code = next_code[sz]++;
      for (unsigned l = sz; l > 0; l--, code >>= 1) rev = (rev << 1) | (code & 1);
      codes[t][i] = (uint16_t)rev;
    }
  }
  void start_static_block() {
    uint8_t* p = sizes[0];
    int i = 0;
    for (; i <= 143; ++i) p[i] = 8;
    for (; i <= 255; ++i) p[i] = 9;
    for (; i <= 279; ++i) p[i] = 7;
    for (; i <= 287; ++i) p[i] = 8;
    memset(sizes[1], 5, 32);
    optimize_table(0, 288, 15, true);
    optimize_table(1, 32, 15, true);
    put(1, 2);
  }
  void start_dynamic_block() {
    static const uint8_t swizzle[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t to_pack[288 + 32], packed[288 + 32], prev = 0xFF;
    unsigned npacked = 0, rle_z = 0, rle_rep = 0;
    count[0][256] = 1;
    optimize_table(0, 288, 15, false);
    optimize_table(1, 32, 15, false);
    int nlit, ndist, nbl;
    for (nlit = 286; nlit > 257; nlit--) if (sizes[0][nlit - 1]) break;
    for (ndist = 30; ndist > 1; ndist--) if (sizes[1][ndist - 1]) break;
    memcpy(to_pack, sizes[0], nlit);
    memcpy(to_pack + nlit, sizes[1], ndist);
    unsigned total = nlit + ndist;
    memset(count[2], 0, sizeof(uint16_t) * 19);
    auto rle_prev = [&]() {
      if (rle_rep) {
        if (rle_rep < 3) { count[2][prev] = (uint16_t)(count[2][prev] + rle_rep); while (rle_rep--) packed[npacked++] = prev; }
        else { count[2][16]++; packed[npacked++] = 16; packed[npacked++] = (uint8_t)(rle_rep - 3); }
        rle_rep = 0;
      }
    };
    auto rle_zero = [&]() {
      if (rle_z) {
        if (rle_z < 3) { count[2][0] = (uint16_t)(count[2][0] + rle_z); while (rle_z--) packed[npacked++] = 0; }
        else if (rle_z <= 10) { count[2][17]++; packed[npacked++] = 17; packed[npacked++] = (uint8_t)(rle_z - 3); }
        else { count[2][18]++; packed[npacked++] = 18; packed[npacked++] = (uint8_t)(rle_z - 11); }
        rle_z = 0;
      }
    };
    for (unsigned i = 0; i < total; i++) {
      uint8_t cs = to_pack[i];
      if (!cs) {
        rle_prev();
        if (++rle_z == 138) rle_zero();
      } else {
        rle_zero();
        if (cs != prev) { rle_prev(); count[2][cs]++; packed[npacked++] = cs; }
        else if (++rle_rep == 6) rle_prev();
      }
      prev = cs;
    }
    if (rle_rep) rle_prev(); else rle_zero();
    optimize_table(2, 19, 7, false);
    put(2, 2);
    put(nlit - 257, 5);
    put(ndist - 1, 5);
    for (nbl = 18; nbl >= 0; nbl--) if (sizes[2][swizzle[nbl]]) break;
    nbl = std::max(4, nbl + 1);
    put(nbl - 4, 4);
    for (int i = 0; i < nbl; i++) put(sizes[2][swizzle[i]], 3);
    for (unsigned k = 0; k < npacked;) {
      unsigned code = packed[k++];
      put(codes[2][code], sizes[2][code]);
      if (code >= 16) put(packed[k++], code == 16 ? 2 : (code == 17 ? 3 : 7));
    }
  }
  void compress_lz_codes() {
    for (const Tok& t : toks) {
      if (t.match) {
        unsigned s, e;
        len_code(t.len_m3, &s, &e);
        static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        put(codes[0][s], sizes[0][s]);
        put((t.len_m3 + 3) - lbase[s - 257], e);   // == match_len & mask(extra) in tdefl's table form
        dist_code(t.dist_m1, &s, &e);
        static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        put(codes[1][s], sizes[1][s]);
        put((t.dist_m1 + 1) - dbase[s], e);
      } else {
        put(codes[0][t.lit], sizes[0][t.lit]);
      }
    }
    put(codes[0][256], sizes[0][256]);
  }
  void flush_block(bool finish) {
    // (the flag byte that was opened but holds no code is given back: code_bytes -= (flags_left == 8) — nothing reads it afterwards)
    if (block_index == 0) {
      // miniz >= 2.2 / miniz_oxide >= 0.4: FLEVEL recovered from the probe count (index in s_tdefl_num_probes), FCHECK makes the 16 bits a multiple of 31
      static const unsigned num_probes[11] = {0, 1, 6, 32, 16, 32, 128, 256, 512, 768, 1500};
      unsigned i = 0, flevel = 3;
      for (; i < 11; i++) if (num_probes[i] == probes) break;
      if (i < 2) flevel = 0; else if (i < 6) flevel = 1; else if (i == 6) flevel = 2;
      unsigned header = (0x78u << 8) | (flevel << 6);
      header += 31 - (header % 31);
      put(0x78, 8); put(old_header ? 0x01 : (header & 0xFF), 8);
    }
    put(finish ? 1 : 0, 1);
    const size_t saved_out = out.size();
    const uint64_t saved_buf = bitbuf;
    const unsigned saved_bits = bits_in;
    if (total_lz_bytes < 48) { static_blocks++; start_static_block(); } else start_dynamic_block();
    compress_lz_codes();
    // if the block got expanded, forget it and send a stored block instead (the data is still in the dictionary)
    if (total_lz_bytes && (out.size() - saved_out + 1u) >= total_lz_bytes && (lookahead_pos - lz_dict_pos) <= dict_size) {
      out.resize(saved_out); bitbuf = saved_buf; bits_in = saved_bits;
      stored_blocks++;
      put(0, 2);
      if (bits_in) put(0, 8 - bits_in);
      put(total_lz_bytes & 0xFFFF, 16);
      put((total_lz_bytes ^ 0xFFFF) & 0xFFFF, 16);
      for (unsigned i = 0; i < total_lz_bytes; ++i) put(stored_src ? stored_src[stored_pos + i] : dict[(lz_dict_pos + i) & DMASK], 8);
    }
    if (finish) {
      if (bits_in) put(0, 8 - bits_in);
      uint32_t a = adler;
      for (int i = 0; i < 4; i++) { put((a >> 24) & 0xFF, 8); a <<= 8; }
    }
    memset(count[0], 0, sizeof count[0]);
    memset(count[1], 0, sizeof count[1]);
    toks.clear();
    code_bytes = 1; flags_left = 8;
    lz_dict_pos += total_lz_bytes;
    stored_pos += total_lz_bytes;
    total_lz_bytes = 0;
    block_index++;
  }
  void find_match(unsigned lpos, unsigned max_dist, unsigned max_match_len, unsigned* pdist, unsigned* plen) {
    unsigned dist = 0, pos = lpos & DMASK, match_len = *plen, probe_pos = pos, next_probe_pos, probe_len;
    unsigned probes_left = max_probes[match_len >= 32];
    if (max_match_len <= match_len) return;
    uint8_t c0 = dict[pos + match_len], c1 = dict[pos + match_len - 1];
    for (;;) {
      for (;;) {
        if (--probes_left == 0) return;
        bool hit = false;
        for (int k = 0; k < 3 && !hit; k++) {
          next_probe_pos = next[probe_pos];
          if (!next_probe_pos || (dist = (uint16_t)(lpos - next_probe_pos)) > max_dist) return;
          probe_pos = next_probe_pos & DMASK;
          if (dict[probe_pos + match_len] == c0 && dict[probe_pos + match_len - 1] == c1) hit = true;
        }
        if (hit) break;
      }
      if (!dist) break;
      const uint8_t *p = dict + pos, *q = dict + probe_pos;
      for (probe_len = 0; probe_len < max_match_len; probe_len++) if (*p++ != *q++) break;
      if (probe_len > match_len) {
        *pdist = dist;
        if ((*plen = match_len = probe_len) == max_match_len) return;
        c0 = dict[pos + match_len]; c1 = dict[pos + match_len - 1];
      }
    }
  }
  void run(const uint8_t* src, size_t n) {
    memset(dict, 0, sizeof dict); memset(next, 0, sizeof next); memset(hash, 0, sizeof hash); memset(count, 0, sizeof count);
    memset(codes, 0, sizeof codes); memset(sizes, 0, sizeof sizes);
    const unsigned flags = probes;  // lazy parsing (levels >= 4; the greedy parser of levels 1..3 is not restated)
    max_probes[0] = 1 + ((flags & 0xFFF) + 2) / 3;
    max_probes[1] = 1 + (((flags & 0xFFF) >> 2) + 2) / 3;
    // Adler-32 of the whole input (tdefl updates it per call; the value at the end is the same)
    {
      uint32_t s1 = 1, s2 = 0;
      for (size_t i = 0; i < n;) {
        size_t blk = std::min<size_t>(5552, n - i);
        for (size_t k = 0; k < blk; k++) { s1 += src[i + k]; s2 += s1; }
        s1 %= 65521; s2 %= 65521; i += blk;
      }
      adler = (s2 << 16) | s1;
    }
    size_t left = n;
    while (left || lookahead_size) {
      // fill the lookahead, inserting every 3-byte string into the hash chains as its last byte arrives
      while (left && lookahead_size < MAXM) {
        uint8_t c = *src++;
        left--;
        unsigned dst = (lookahead_pos + lookahead_size) & DMASK;
        dict[dst] = c;
        if (dst < MAXM - 1) dict[DICT + dst] = c;
        if (++lookahead_size + dict_size >= MINM) {
          unsigned ins = lookahead_pos + (lookahead_size - 1) - 2;
          unsigned h = ((dict[ins & DMASK] << (HSHIFT * 2)) ^ (dict[(ins + 1) & DMASK] << HSHIFT) ^ c) & (HSIZE - 1);
          next[ins & DMASK] = hash[h];
          hash[h] = (uint16_t)ins;
        }
      }
      dict_size = std::min(DICT - lookahead_size, dict_size);
      if (left == 0 && lookahead_size == 0) break;
      // (no-flush calls stop here while the lookahead is short; with the whole input in hand the lookahead is full until the tail)
      unsigned len_to_move = 1, cur_match_dist = 0, cur_match_len = saved_match_len ? saved_match_len : (MINM - 1), cur_pos = lookahead_pos & DMASK;
      find_match(lookahead_pos, dict_size, lookahead_size, &cur_match_dist, &cur_match_len);
      if ((cur_match_len == MINM && cur_match_dist >= 8u * 1024u) || cur_pos == cur_match_dist) cur_match_dist = cur_match_len = 0;
      if (saved_match_len) {
        if (cur_match_len > saved_match_len) {
          record_literal((uint8_t)saved_lit);
          if (cur_match_len >= 128) { record_match(cur_match_len, cur_match_dist); saved_match_len = 0; len_to_move = cur_match_len; }
          else { saved_lit = dict[cur_pos]; saved_match_dist = cur_match_dist; saved_match_len = cur_match_len; }
        } else {
          record_match(saved_match_len, saved_match_dist);
          len_to_move = saved_match_len - 1;
          saved_match_len = 0;
        }
      } else if (!cur_match_dist) {
        record_literal(dict[cur_pos]);
      } else if (cur_match_len >= 128) {
        record_match(cur_match_len, cur_match_dist);
        len_to_move = cur_match_len;
      } else {
        saved_lit = dict[cur_pos]; saved_match_dist = cur_match_dist; saved_match_len = cur_match_len;
      }
      lookahead_pos += len_to_move;
      lookahead_size -= len_to_move;
      dict_size = std::min(dict_size + len_to_move, DICT);
      if (code_bytes > LZBUF - 8 || (total_lz_bytes > 31 * 1024 && ((code_bytes * 115) >> 7) >= total_lz_bytes)) flush_block(false);
    }
    // finish: a match still held is emitted by the parser above before the lookahead runs dry (its len_to_move consumes it)
    flush_block(true);
  }
};

// ---- the restatements: the rules of csrc/tdefl_rules.hpp applied on the host
// The parser's look-up at p (init == 2: it holds nothing; else the length it holds) answered from the tables of one segment: A and B are
// those of positions [first, first + count), prevA is A[first - 1]. A when the parser is free; B when A[p - 1] is held at exactly this
// length; else — a lazy chain of three or more whose held length is not A[p - 1]'s — searched on the spot over links() = Lbase with
// Lbase[q - Lfirst] = L[q], asked for on the first such look-up only.
template <typename Links>
struct TableLookup {
  const uint8_t* D;
  size_t n, first;
  const uint32_t *A, *B;
  uint32_t prevA;
  Links links;
  size_t Lfirst;
  const unsigned* mp;
  uint64_t lookups = 0, fallbacks = 0;
  uint32_t operator()(size_t p, unsigned init) {
    lookups++;
    if (init == tdefl::MINM - 1) return A[p - first];
    const uint32_t aprev = p > first ? A[p - 1 - first] : prevA;
    if (p && tdefl::held(aprev, p - 1) && (aprev >> 16) == init) return B[p - first];
    fallbacks++;
    return tdefl::find(D, n, links(), Lfirst, p, init, mp);
  }
};
template <typename Links>
TableLookup<Links> table_lookup(const uint8_t* D, size_t n, size_t first, const uint32_t* A, const uint32_t* B, uint32_t prevA, Links links, size_t Lfirst,
                                const unsigned* mp) {
  return TableLookup<Links>{D, n, first, A, B, prevA, links, Lfirst, mp};
}

// record_literal, record_match, the block check and flush_block of Tdefl, one token at a time: no tables, no dictionary, no search. The
// two numbers flush_block's stored-block test reads are those of the parser's step the token closes: the step at p with lookahead
// la = min(258, n - p) starts from dict_size = min(p, 32768 - la) and moves m positions.
struct Coder {
  Tdefl d;
  size_t n, pos = 0;        // input length, position of the next token
  uint32_t s1 = 1, s2 = 0;  // Adler-32 so far
  size_t adler_pos = 0;
  uint64_t full_blocks = 0, ratio_blocks = 0;  // blocks ended by the code-buffer rule / the 115/128 rule
  Coder(size_t n_, unsigned probes, bool old_header) : n(n_) {
    memset(d.count, 0, sizeof d.count); memset(d.codes, 0, sizeof d.codes); memset(d.sizes, 0, sizeof d.sizes);
    d.old_header = old_header;
    d.probes = probes & 0xFFF;
  }
  // D[0, end) has arrived: Adler-32 of the input as it arrives; the bytes of a stored block come from D
  void arrive(const uint8_t* D, size_t end) {
    d.stored_src = D;
    while (adler_pos < end) {
      const size_t blk = std::min<size_t>(5552, end - adler_pos);
      for (size_t k = 0; k < blk; k++) { s1 += D[adler_pos + k]; s2 += s1; }
      s1 %= 65521; s2 %= 65521; adler_pos += blk;
    }
  }
  // inlined into its callers' loops by force: left as a call it costs the coder 5-10 % (bench/deflate_host_probe.cc, time 16)
  __attribute__((always_inline)) void token(uint32_t t) {
    const unsigned len = tdefl::tok_len(t);
    const size_t at = pos;  // where the token starts
    if (!len) d.record_literal((uint8_t)t); else d.record_match(len, tdefl::tok_dist(t));
    pos += tdefl::tok_input_bytes(t);
    if (!(t & TOK_CHECK)) return;
    uint64_t lookahead_pos;
    uint32_t dict_size;
    tdefl::tok_step(t, at, n, &lookahead_pos, &dict_size);  // the parser's step this token closes
    d.lookahead_pos = (unsigned)lookahead_pos;
    d.dict_size = dict_size;
    const tdefl::BlockRule rule = tdefl::block_check(d.code_bytes, d.total_lz_bytes);
    if (rule == tdefl::RULE_FULL) { full_blocks++; d.flush_block(false); }
    else if (rule == tdefl::RULE_RATIO) { ratio_blocks++; d.flush_block(false); }
  }
  std::vector<uint8_t> finish() {
    d.adler = (s2 << 16) | s1;
    d.flush_block(true);
    return std::move(d.out);
  }
};
}  // namespace

void deflate_links_host(const uint8_t* D, size_t n, uint16_t* L) {
  std::vector<uint16_t> head((size_t)1 << tdefl::HBITS, 0);
  for (size_t p = 0; p < n; p++) {
    if (p + 2 >= n) { L[p] = 0; continue; }
    const unsigned h = tdefl::hash3(D + p);
    L[p] = head[h];
    head[h] = (uint16_t)p;
  }
}
void deflate_matches_host(const uint8_t* D, size_t n, unsigned probes, const uint16_t* L, uint32_t* A, uint32_t* B) {
  std::vector<uint16_t> own;
  if (!L) { own.resize(n ? n : 1); deflate_links_host(D, n, own.data()); L = own.data(); }
  unsigned mp[2];
  tdefl::probe_budget(probes, mp);
  for (size_t p = 0; p < n; p++) A[p] = tdefl::find(D, n, L, 0, p, tdefl::MINM - 1, mp);
  for (size_t p = 0; p < n; p++) B[p] = p && tdefl::held(A[p - 1], p - 1) ? tdefl::find(D, n, L, 0, p, A[p - 1] >> 16, mp) : 0;
}

// Fed segment by segment, so that it can run behind the device search. What a segment needs of those before it: the walk's state, A's last
// entry, and for a search on the spot the last 32768 links (zeros before position 0, which no search reaches).
struct MatchParser::Impl {
  Coder coder;
  tdefl::WalkState w{0, 0, 0};
  uint32_t prevA = 0;                                         // A[first - 1] of the segment being parsed
  std::vector<uint16_t> ltail = std::vector<uint16_t>(tdefl::DICT);  // L[first - 32768, first)
  std::vector<uint16_t> lwin;                                 // ltail followed by the segment's links, built on the segment's first fallback
  unsigned mp[2];
  Impl(size_t n, unsigned probes, bool old_header) : coder(n, probes, old_header) { tdefl::probe_budget(probes, mp); }
};
MatchParser::MatchParser(size_t n, unsigned probes, bool old_header) : m(new Impl(n, probes, old_header)) {}
MatchParser::~MatchParser() { delete m; }
void MatchParser::parse(const uint8_t* D, size_t first, size_t count, const uint16_t* L, const uint32_t* A, const uint32_t* B) {
  Impl& s = *m;
  const size_t end = first + count;
  s.coder.arrive(D, end);
  bool lwin_built = false;
  auto links = [&]() -> const uint16_t* {
    if (!lwin_built) {
      s.lwin.assign(s.ltail.begin(), s.ltail.end());
      s.lwin.insert(s.lwin.end(), L, L + count);
      lwin_built = true;
    }
    return s.lwin.data();
  };
  auto lookup = table_lookup(D, s.coder.n, first, A, B, s.prevA, links, first - tdefl::DICT, s.mp);
  auto emit = [&](size_t, uint32_t t) { s.coder.token(t); };
  while (s.w.q < end) tdefl::walk(D, s.w, end, lookup, emit);
  lookups += lookup.lookups; fallbacks += lookup.fallbacks;
  if (count) {
    s.prevA = A[count - 1];
    if (count < tdefl::DICT) s.ltail.erase(s.ltail.begin(), s.ltail.begin() + count); else s.ltail.clear();
    s.ltail.insert(s.ltail.end(), L + count - std::min<size_t>(count, tdefl::DICT), L + count);
  }
}
std::vector<uint8_t> MatchParser::finish() { return m->coder.finish(); }
std::vector<uint8_t> zlib_from_matches(const uint8_t* D, size_t n, const uint16_t* L, const uint32_t* A, const uint32_t* B, unsigned probes, bool old_header,
                                       uint64_t* lookups, uint64_t* fallbacks) {
  std::vector<uint16_t> own;
  if (!L) { own.resize(n ? n : 1); deflate_links_host(D, n, own.data()); L = own.data(); }
  MatchParser mp(n, probes, old_header);
  mp.parse(D, 0, n, L, A, B);
  if (lookups) *lookups = mp.lookups;
  if (fallbacks) *fallbacks = mp.fallbacks;
  return mp.finish();
}

size_t deflate_tokens_host(const uint8_t* D, size_t n, unsigned probes, const size_t geom[3], uint32_t* tokens, uint64_t counters[TOKC_COUNT]) {
  std::vector<uint16_t> L(n ? n : 1);
  std::vector<uint32_t> A(n ? n : 1), B(n ? n : 1);
  deflate_links_host(D, n, L.data());
  deflate_matches_host(D, n, probes, L.data(), A.data(), B.data());
  unsigned mp[2];
  tdefl::probe_budget(probes, mp);
  uint64_t own[TOKC_COUNT];
  uint64_t* C = counters ? counters : own;
  memset(C, 0, sizeof own);
  const size_t tile = geom && geom[0] ? geom[0] : 1024, group = tile * (geom && geom[1] ? geom[1] : 64), seg = geom && geom[2] ? geom[2] : (n ? n : 1);
  size_t ntok = 0, first = 0;
  auto lookup = table_lookup(D, n, 0, A.data(), B.data(), 0, [&] { return L.data(); }, 0, mp);
  auto emit = [&](size_t pos, uint32_t t) {
    tokens[ntok++] = t;
    const unsigned len = tdefl::tok_len(t);
    if (len) {
      const size_t a = pos - first, b = a + len - 1;  // a match starts in the segment under way (or one position before it: the prologue's)
      if (pos >= first && b < seg && first + b < n) {
        if (a / tile != b / tile) C[TOKC_SPAN_TILE]++;
        if (a / group != b / group) C[TOKC_SPAN_GROUP]++;
      }
    }
  };
  tdefl::WalkState w{0, 0, 0};
  for (; first < n; first += seg) {
    const size_t end = std::min(n, first + seg);
    if (w.sl) C[TOKC_SEAM_HELD]++;  // the segment's entry is a held match: its first walk is resolved from the carried state
    while (w.q < end) {
      const size_t p = w.q, before = ntok;
      const bool was_free = w.sl == 0;
      tdefl::walk(D, w, end, lookup, emit);
      C[TOKC_WALKS]++;
      if (was_free && !w.sl) C[TOKC_MAX_JUMP] = std::max<uint64_t>(C[TOKC_MAX_JUMP], w.q - p);
      if (ntok - before == 1 && was_free && tdefl::tok_len(tokens[before]) >= tdefl::TAKE) C[TOKC_FREE_LONG]++;
      if (ntok - before >= 2 && !(tokens[ntok - 2] & TOK_CHECK)) C[TOKC_LIT_AND_LONG]++;
    }
  }
  C[TOKC_LOOKUPS] = lookup.lookups; C[TOKC_FALLBACKS] = lookup.fallbacks;
  C[TOKC_TOKENS] = ntok;
  return ntok;
}

struct TokenCoder::Impl {
  Coder coder;
};
TokenCoder::TokenCoder(size_t n, unsigned probes, bool old_header) : m(new Impl{Coder(n, probes, old_header)}) {}
TokenCoder::~TokenCoder() { delete m; }
void TokenCoder::code(const uint8_t* D, size_t bytes_end, const uint32_t* tokens, size_t ntok) {
  Coder& c = m->coder;
  c.arrive(D, bytes_end);
  for (size_t i = 0; i < ntok; i++) c.token(tokens[i]);
  tokens_coded += ntok; full_blocks = c.full_blocks; ratio_blocks = c.ratio_blocks;
}
std::vector<uint8_t> TokenCoder::finish() {
  std::vector<uint8_t> z = m->coder.finish();
  static_blocks = m->coder.d.static_blocks; stored_blocks = m->coder.d.stored_blocks;
  return z;
}
std::vector<uint8_t> zlib_from_tokens(const uint8_t* D, size_t n, const uint32_t* tokens, size_t ntok, unsigned probes, bool old_header, size_t piece,
                                      uint64_t blocks[4]) {
  TokenCoder tc(n, probes, old_header);
  if (!piece) piece = ntok ? ntok : 1;
  for (size_t i = 0; i < ntok; i += piece) tc.code(D, n, tokens + i, std::min(piece, ntok - i));
  if (!ntok) tc.code(D, n, tokens, 0);
  std::vector<uint8_t> z = tc.finish();
  if (blocks) { blocks[0] = tc.full_blocks; blocks[1] = tc.ratio_blocks; blocks[2] = tc.stored_blocks; blocks[3] = tc.static_blocks; }
  return z;
}

// ---- the coder split as the device runs it (csrc/deflate_emit.hip): block records from prefix sums of token costs, then tables and bit
// offsets per block from its histogram alone, then every token's bits as an independent item
namespace {
void or_bits(std::vector<uint8_t>& z, uint64_t off, uint64_t v, unsigned nb) {  // v's low nb bits at bit `off`, first bit lowest
  for (unsigned done = 0; done < nb;) {
    const unsigned sh = (unsigned)((off + done) & 7), take = std::min(8 - sh, nb - done);
    z[(off + done) >> 3] |= (uint8_t)(((v >> done) & ((1u << take) - 1)) << sh);
    done += take;
  }
}
unsigned len_extra_bits(unsigned sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) / 4; }
unsigned dist_extra_bits(unsigned sym) { return sym < 4 ? 0 : sym / 2 - 1; }
}  // namespace

size_t deflate_blocks_host(const uint32_t* tokens, size_t ntok, size_t n, size_t segment, uint64_t* records, uint16_t* hist, size_t cap,
                           uint64_t counters[BLKC_COUNT]) {
  uint64_t own[BLKC_COUNT];
  uint64_t* C = counters ? counters : own;
  memset(C, 0, sizeof own);
  if (!segment) segment = n ? n : 1;
  const size_t nseg = n ? (n + segment - 1) / segment : 1;
  std::vector<uint32_t> list;          // the open block's tokens, then the segment's
  std::vector<uint64_t> code, lz;      // inclusive sums of the list's code bytes and input bytes
  uint64_t gtok = 0, pos0 = 0;         // list[0]'s index in the whole token list, and its input position
  size_t nb = 0, next = 0, span = 1;
  uint64_t tpos = 0;                   // where token `next` starts
  for (size_t s = 0; s < nseg; s++) {
    const bool last = s + 1 == nseg;
    const uint64_t end_pos = last ? n : (uint64_t)(s + 1) * segment;
    if (s && !list.empty()) { C[BLKC_SEAM_OPEN]++; span++; }
    while (next < ntok && (tpos < end_pos || last)) { list.push_back(tokens[next]); tpos += tdefl::tok_input_bytes(tokens[next]); next++; }
    const size_t m = list.size();
    code.resize(m); lz.resize(m);
    for (size_t i = 0; i < m; i++) {
      code[i] = (i ? code[i - 1] : 0) + tdefl::tok_code_bytes(list[i]);
      lz[i] = (i ? lz[i - 1] : 0) + tdefl::tok_input_bytes(list[i]);
    }
    size_t start = 0;
    auto close = [&](size_t end, tdefl::BlockRule rule) {  // the block list[start, end)
      if (nb >= cap) throw Error("deflate_blocks_host: more blocks than the caller's arrays hold");
      const size_t k = end - start;
      if (k > tdefl::BLOCK_TOKENS) throw Error("deflate_blocks_host: a block of more than 58249 tokens");
      const uint64_t lz0 = start ? lz[start - 1] : 0, total = end ? lz[end - 1] - lz0 : 0;
      uint64_t la = 0;
      uint32_t ds = 0;
      if (k) {
        const uint64_t at = pos0 + lz[end - 1] - tdefl::tok_input_bytes(list[end - 1]);
        tdefl::tok_step(list[end - 1], at, n, &la, &ds);
        la = (uint32_t)(la - (pos0 + lz0));
      }
      uint64_t* r = records + BLOCK_REC * nb;
      r[0] = gtok + start; r[1] = k; r[2] = total; r[3] = rule; r[4] = la; r[5] = ds;
      uint16_t* h = hist + BLOCK_HIST * nb;
      memset(h, 0, sizeof(uint16_t) * BLOCK_HIST);
      for (size_t i = start; i < end; i++) {
        const unsigned len = tdefl::tok_len(list[i]);
        if (!len) { h[list[i] & 0xFF]++; continue; }
        unsigned sym, ne, ev;
        tdefl::len_symbol(len, &sym, &ne, &ev); h[sym]++;
        tdefl::dist_symbol(tdefl::tok_dist(list[i]), &sym, &ne, &ev); h[288 + sym]++;
      }
      C[BLKC_MAX_TOKENS] = std::max<uint64_t>(C[BLKC_MAX_TOKENS], k);
      C[BLKC_MAX_SPAN] = std::max<uint64_t>(C[BLKC_MAX_SPAN], span);
      if (rule == tdefl::RULE_FULL) C[BLKC_FULL]++;
      if (rule == tdefl::RULE_RATIO) C[BLKC_RATIO]++;
      if (rule == tdefl::RULE_FINISH && !k) C[BLKC_EMPTY_FINAL]++;
      if (rule != tdefl::RULE_FINISH && end == m && !last) C[BLKC_SEAM_AT_BOUNDARY]++;
      nb++; span = 1; start = end;
    };
    for (;;) {  // the chain: from a block's start, the first TOK_CHECK token at which the check fires
      const uint64_t c0 = start ? code[start - 1] : 0, l0 = start ? lz[start - 1] : 0;
      size_t hit = m;
      tdefl::BlockRule rule = tdefl::RULE_NONE;
      for (size_t i = start; i < m && hit == m; i++)
        if ((list[i] & TOK_CHECK) && (rule = tdefl::block_check(tdefl::code_bytes_after(code[i] - c0, i - start + 1), lz[i] - l0)) != tdefl::RULE_NONE) hit = i;
      if (hit == m) break;
      close(hit + 1, rule);
    }
    if (last) close(m, tdefl::RULE_FINISH);
    gtok += start; pos0 += start ? lz[start - 1] : 0;
    list.erase(list.begin(), list.begin() + start);
  }
  return nb;
}

struct BlockPlanner::Impl {
  Tdefl d;
};
BlockPlanner::BlockPlanner(unsigned probes, bool old_header) : m(new Impl()) {
  Tdefl& d = m->d;
  memset(d.count, 0, sizeof d.count); memset(d.codes, 0, sizeof d.codes); memset(d.sizes, 0, sizeof d.sizes);
  // the zlib header as flush_block writes it before the first block
  static const unsigned num_probes[11] = {0, 1, 6, 32, 16, 32, 128, 256, 512, 768, 1500};
  unsigned i = 0, flevel = 3;
  for (; i < 11; i++) if (num_probes[i] == (probes & 0xFFF)) break;
  if (i < 2) flevel = 0; else if (i < 6) flevel = 1; else if (i == 6) flevel = 2;
  unsigned header = (0x78u << 8) | (flevel << 6);
  header += 31 - (header % 31);
  head[0] = 0x78; head[1] = old_header ? 0x01 : (uint8_t)(header & 0xFF);
}
BlockPlanner::~BlockPlanner() { delete m; }
void BlockPlanner::plan(const uint64_t* rec, const uint16_t* hist, BlockPlan& p) {
  Tdefl& d = m->d;
  const bool finish = rec[3] == tdefl::RULE_FINISH;
  const uint64_t total = rec[2];
  d.out.clear(); d.bitbuf = 0; d.bits_in = 0;
  for (int i = 0; i < 288; i++) d.count[0][i] = hist[i];
  for (int i = 0; i < 32; i++) d.count[1][i] = hist[288 + i];
  d.total_lz_bytes = (unsigned)total;
  d.put(finish ? 1 : 0, 1);
  const bool is_static = total < 48;
  if (is_static) d.start_static_block(); else d.start_dynamic_block();
  const uint32_t hdr_bits = (uint32_t)(8 * d.out.size() + d.bits_in);
  uint64_t tokbits = 0;  // the coded length from the histogram alone
  for (unsigned i = 0; i < 288; i++)
    if (i != 256) tokbits += (uint64_t)hist[i] * (d.sizes[0][i] + len_extra_bits(i));
  for (unsigned i = 0; i < 32; i++) tokbits += (uint64_t)hist[288 + i] * (d.sizes[1][i] + dist_extra_bits(i));
  const uint64_t P0 = bitpos, end_coded = P0 + hdr_bits + tokbits + d.sizes[0][256];
  // flush_block's test counts whole bytes written since the block's first bit went in: it depends on the bits pending before the block
  const bool stored = total && (end_coded / 8 - (P0 + 1) / 8 + 1) >= total && rec[4] <= rec[5];
  memset(p.hdr, 0, sizeof p.hdr);
  p.bit_off = P0; p.src = src; p.total = total;
  if (stored) {
    const unsigned pad = (unsigned)((8 - (P0 + 3) % 8) % 8);
    p.kind = BLOCK_STORED; p.hdr_bits = 3 + pad + 32;
    std::vector<uint8_t> h(sizeof p.hdr, 0);
    or_bits(h, 0, finish ? 1 : 0, 3);
    or_bits(h, 3 + pad, total & 0xFFFF, 16);
    or_bits(h, 3 + pad + 16, (total ^ 0xFFFF) & 0xFFFF, 16);
    memcpy(p.hdr, h.data(), sizeof p.hdr);
    p.tok_off = P0 + p.hdr_bits; p.eob_off = 0; p.end_off = p.tok_off + 8 * total;
    memset(p.table, 0, sizeof p.table);
    stored_blocks++;
    if (P0 % 8) stored_after_midbyte++;
  } else {
    if ((hdr_bits + 7) / 8 > sizeof p.hdr) throw Error("BlockPlanner: a block header longer than its slot");
    p.kind = is_static ? BLOCK_STATIC : BLOCK_DYNAMIC; p.hdr_bits = hdr_bits;
    if (!d.out.empty()) memcpy(p.hdr, d.out.data(), d.out.size());  // a static block's three bits fill no byte
    if (d.bits_in) p.hdr[d.out.size()] = (uint8_t)d.bitbuf;
    p.tok_off = P0 + hdr_bits; p.eob_off = p.tok_off + tokbits; p.end_off = end_coded;
    for (unsigned i = 0; i < 288; i++) p.table[i] = d.codes[0][i] | ((uint32_t)d.sizes[0][i] << 16);
    for (unsigned i = 0; i < 32; i++) p.table[288 + i] = d.codes[1][i] | ((uint32_t)d.sizes[1][i] << 16);
    if (is_static) static_blocks++;
  }
  bitpos = p.end_off; src += total; blocks++;
}
void BlockPlanner::finish(std::vector<uint8_t>& z, uint32_t adler) const {
  z.resize(stream_bytes(), 0);
  z[0] |= head[0]; z[1] |= head[1];
  for (int i = 0; i < 4; i++) z[z.size() - 4 + i] = (uint8_t)(adler >> (24 - 8 * i));
}

std::vector<uint8_t> zlib_from_blocks(const uint64_t* records, const uint16_t* hist, size_t nblocks, const uint32_t* tokens, const uint8_t* D, size_t n,
                                      unsigned probes, bool old_header, uint64_t stats[3]) {
  BlockPlanner bp(probes, old_header);
  std::vector<BlockPlan> plans(nblocks);
  for (size_t b = 0; b < nblocks; b++) bp.plan(records + BLOCK_REC * b, hist + BLOCK_HIST * b, plans[b]);  // tables, lengths, decisions, offsets: block by block
  std::vector<uint8_t> z(bp.stream_bytes(), 0);
  std::vector<uint32_t> off;
  for (size_t b = 0; b < nblocks; b++) {  // the bits: every header, token and byte an item of its own, ORed in at its offset
    const BlockPlan& p = plans[b];
    const uint64_t* r = records + BLOCK_REC * b;
    for (unsigned i = 0; 8 * i < p.hdr_bits; i++) or_bits(z, p.bit_off + 8 * i, p.hdr[i], std::min(8u, p.hdr_bits - 8 * i));
    if (p.kind == BLOCK_STORED) {
      if (p.src + p.total > n) throw Error("zlib_from_blocks: a stored block past the input's end");
      memcpy(z.data() + p.tok_off / 8, D + p.src, p.total);
      continue;
    }
    const uint32_t* t = tokens + r[0];
    off.assign(r[1] + 1, 0);
    for (size_t i = 0; i < r[1]; i++) off[i + 1] = off[i] + tdefl::tok_nbits(t[i], p.table);  // the exclusive scan of the lengths
    if (p.tok_off + off[r[1]] != p.eob_off) throw Error("zlib_from_blocks: the tokens' bits differ from the histogram's");
    for (size_t i = 0; i < r[1]; i++) {
      uint64_t v;
      const unsigned nbits = tdefl::tok_bits(t[i], p.table, &v);
      or_bits(z, p.tok_off + off[i], v, nbits);
    }
    or_bits(z, p.eob_off, p.table[256] & 0xFFFF, p.table[256] >> 16);
  }
  uint32_t s1 = 1, s2 = 0;
  for (size_t i = 0; i < n;) {
    const size_t blk = std::min<size_t>(5552, n - i);
    for (size_t k = 0; k < blk; k++) { s1 += D[i + k]; s2 += s1; }
    s1 %= 65521; s2 %= 65521; i += blk;
  }
  bp.finish(z, (s2 << 16) | s1);
  if (stats) { stats[0] = bp.stored_blocks; stats[1] = bp.static_blocks; stats[2] = bp.stored_after_midbyte; }
  return z;
}

std::vector<uint8_t> zlib_miniz_probes(const uint8_t* data, size_t n, unsigned probes, bool old_header) {
  std::unique_ptr<Tdefl> d(new Tdefl());
  d->old_header = old_header;
  d->probes = probes & 0xFFF;
  d->run(data, n);
  return std::move(d->out);
}
std::vector<uint8_t> zlib_level6_miniz(const uint8_t* data, size_t n, bool old_header) { return zlib_miniz_probes(data, n, 128, old_header); }

}  // namespace spz
