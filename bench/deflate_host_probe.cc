// Stand-alone host program over spartan_amd/host/deflate.cc (no device, no Python): two uses.
//   check   the token model, the token coder and the parser over match tables (whole, and fed in segments of 32 768 and 49 999 positions as
//           it is behind the device search), and the coder split into block records, per-block plans and independent token items (found in
//           segments of 32 768 and 49 999 positions as the device finds them) against the sequential deflater on a few inputs; built with
//           sanitizers this is the host-code sanitizer run of the deflate restatements:
//             clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//                 bench/deflate_host_probe.cc spartan_amd/host/deflate.cc -o deflate_host_probe_san && ./deflate_host_probe_san check
//   time K  where the host's time goes on bincode(shape) of a 2^K instance (three entries a row and matrix, random scalars: the bytes of
//           bench/digest_probe.py's instance in kind): the sequential deflater, the parser over match tables with its coding
//           (zlib_from_matches: what runs behind the device search), the token coder alone (zlib_from_tokens: what runs behind the device
//           parse), the block records and the stream from them (what digest.device = 3 leaves the host is BlockPlanner alone, timed by itself)
//           and Adler-32 alone. Build with -O2 and without sanitizers.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../spartan_amd/host/libspartan.hpp"

using namespace spz;
namespace {
uint64_t g_state = 88172645463325252ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
double now_ms() { return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

std::vector<uint8_t> shape_like(size_t log2) {
  const size_t rows = (size_t)1 << log2, per = 3;
  std::vector<uint8_t> b;
  auto u64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) b.push_back((uint8_t)(v >> (8 * i))); };
  u64(rows); u64(rows); u64(10);
  for (int m = 0; m < 3; m++) {
    u64(log2); u64(log2 + 1); u64(rows * per);
    for (size_t e = 0; e < rows * per; e++) {
      u64(e / per); u64(rnd() % rows);
      for (int w = 0; w < 4; w++) u64(w == 3 ? rnd() >> 4 : rnd());
    }
  }
  return b;
}
std::vector<uint8_t> words(size_t n, unsigned alphabet) {
  std::vector<std::vector<uint8_t>> w(40);
  for (auto& x : w) { x.resize(3 + rnd() % 9); for (auto& c : x) c = (uint8_t)('a' + rnd() % alphabet); }
  std::vector<uint8_t> b;
  while (b.size() < n) { const auto& x = w[rnd() % w.size()]; b.insert(b.end(), x.begin(), x.end()); if (rnd() % 5 == 0) b.push_back((uint8_t)('a' + rnd() % alphabet)); }
  b.resize(n);
  return b;
}

int check() {
  std::vector<std::pair<std::string, std::vector<uint8_t>>> inputs;
  inputs.push_back({"empty", {}});
  inputs.push_back({"two bytes", {1, 2}});
  inputs.push_back({"zeros 70000", std::vector<uint8_t>(70000, 0)});
  inputs.push_back({"words/4 70001", words(70001, 4)});
  inputs.push_back({"words/20 131077", words(131077, 20)});
  std::vector<uint8_t> r(66000);
  for (auto& c : r) c = (uint8_t)rnd();
  inputs.push_back({"random 66000", r});
  inputs.push_back({"shape 2^9", shape_like(9)});
  std::vector<uint8_t> mixed = words(40000, 20);  // a coded block that runs into random bytes, then stored blocks
  for (int i = 0; i < 130000; i++) mixed.push_back((uint8_t)rnd());
  inputs.push_back({"words+random", mixed});
  int bad = 0;
  for (const auto& in : inputs) {
    const std::vector<uint8_t>& x = in.second;
    for (unsigned probes : {16u, 128u, 1500u}) {
      const size_t geom[3] = {512, 2, 32768};
      std::vector<uint32_t> tok(x.size() ? x.size() : 1);
      uint64_t cnt[TOKC_COUNT], blocks[4];
      const size_t k = deflate_tokens_host(x.data(), x.size(), probes, geom, tok.data(), cnt);
      const std::vector<uint8_t> want = zlib_miniz_probes(x.data(), x.size(), probes);
      const bool ok = zlib_from_tokens(x.data(), x.size(), tok.data(), k, probes, false, 0, blocks) == want &&
                      zlib_from_tokens(x.data(), x.size(), tok.data(), k, probes, false, 777) == want;
      // the parser over host tables, fed as digest.cc feeds it behind the device search: segment by segment
      const size_t n = x.size();
      std::vector<uint16_t> L(n ? n : 1);
      std::vector<uint32_t> A(n ? n : 1), B(n ? n : 1);
      deflate_links_host(x.data(), n, L.data());
      deflate_matches_host(x.data(), n, probes, L.data(), A.data(), B.data());
      for (size_t seg : {(size_t)32768, (size_t)49999}) {
        MatchParser mp(n, probes, false);
        for (size_t first = 0; first < n; first += seg) mp.parse(x.data(), first, std::min(seg, n - first), L.data() + first, A.data() + first, B.data() + first);
        const bool same = mp.finish() == want;
        printf("%-16s %4u probes: MatchParser in segments of %5zu: %8llu look-ups, %6llu searched on the spot: %s\n", in.first.c_str(), probes, seg,
               (unsigned long long)mp.lookups, (unsigned long long)mp.fallbacks, same ? "equal" : "DIFFERS");
        bad += !same;
      }
      for (size_t seg : {(size_t)0, (size_t)32768, (size_t)49999}) {  // the coder split as the device runs it
        const size_t cap = k / 11306 + 4;
        std::vector<uint64_t> rec(BLOCK_REC * cap);
        std::vector<uint16_t> hist(BLOCK_HIST * cap);
        uint64_t bc[BLKC_COUNT], st3[3];
        const size_t nb = deflate_blocks_host(tok.data(), k, n, seg, rec.data(), hist.data(), cap, bc);
        const bool same = zlib_from_blocks(rec.data(), hist.data(), nb, tok.data(), x.data(), n, probes, false, st3) == want;
        printf("%-16s %4u probes: blocks in segments of %5zu: %3zu (full %llu, ratio %llu, stored %llu, static %llu, stored off a byte %llu), open over %llu seams, "
               "widest span %llu: %s\n", in.first.c_str(), probes, seg, nb, (unsigned long long)bc[BLKC_FULL], (unsigned long long)bc[BLKC_RATIO],
               (unsigned long long)st3[0], (unsigned long long)st3[1], (unsigned long long)st3[2], (unsigned long long)bc[BLKC_SEAM_OPEN],
               (unsigned long long)bc[BLKC_MAX_SPAN], same ? "equal" : "DIFFERS");
        bad += !same;
      }
      printf("%-16s %4u probes: %8zu tokens, %6llu look-ups searched on the spot, longest jump %3llu, blocks full/ratio/stored/static %llu/%llu/%llu/%llu: %s\n",
             in.first.c_str(), probes, k, (unsigned long long)cnt[TOKC_FALLBACKS], (unsigned long long)cnt[TOKC_MAX_JUMP], (unsigned long long)blocks[0],
             (unsigned long long)blocks[1], (unsigned long long)blocks[2], (unsigned long long)blocks[3], ok ? "equal" : "DIFFERS");
      bad += !ok;
    }
  }
  return bad ? 1 : 0;
}

int time_phases(size_t log2) {
  const std::vector<uint8_t> x = shape_like(log2);
  const size_t n = x.size();
  printf("# bincode(shape)-like bytes of a 2^%zu instance: %.1f MB; one host thread; ms\n", log2, n / 1e6);
  double t0 = now_ms();
  const std::vector<uint8_t> want = zlib_level6_miniz(x.data(), n);
  printf("sequential deflater (search, parse, coding)            %10.1f\n", now_ms() - t0);
  std::vector<uint16_t> L(n);
  std::vector<uint32_t> A(n), B(n), tok(n);
  t0 = now_ms();
  deflate_links_host(x.data(), n, L.data());
  deflate_matches_host(x.data(), n, 128, L.data(), A.data(), B.data());
  printf("match tables on the host (the device's share, form 1)   %10.1f\n", now_ms() - t0);
  t0 = now_ms();
  uint64_t lookups = 0, fallbacks = 0;
  const bool ok1 = zlib_from_matches(x.data(), n, L.data(), A.data(), B.data(), 128, false, &lookups, &fallbacks) == want;
  const double t_matches = now_ms() - t0;
  printf("parser over the tables + coding (zlib_from_matches)     %10.1f   %s, %llu look-ups\n", t_matches, ok1 ? "equal" : "DIFFERS", (unsigned long long)lookups);
  const size_t k = deflate_tokens_host(x.data(), n, 128, nullptr, tok.data(), nullptr);
  t0 = now_ms();
  const bool ok2 = zlib_from_tokens(x.data(), n, tok.data(), k, 128, false) == want;
  const double t_tokens = now_ms() - t0;
  printf("token coder alone (zlib_from_tokens)                    %10.1f   %s, %zu tokens\n", t_tokens, ok2 ? "equal" : "DIFFERS", k);
  {
    const size_t cap = k / 11306 + 4;
    std::vector<uint64_t> rec(BLOCK_REC * cap);
    std::vector<uint16_t> hist(BLOCK_HIST * cap);
    t0 = now_ms();
    const size_t nb = deflate_blocks_host(tok.data(), k, n, 4194304, rec.data(), hist.data(), cap, nullptr);
    const double t_rec = now_ms() - t0;
    t0 = now_ms();
    const bool ok3 = zlib_from_blocks(rec.data(), hist.data(), nb, tok.data(), x.data(), n, 128, false, nullptr) == want;
    const double t_blocks = now_ms() - t0;
    t0 = now_ms();
    BlockPlanner bp(128, false);
    BlockPlan p;
    for (size_t b = 0; b < nb; b++) bp.plan(rec.data() + BLOCK_REC * b, hist.data() + BLOCK_HIST * b, p);
    printf("block records on the host (the device's share, form 3)  %10.1f   %zu blocks\n", t_rec, nb);
    printf("stream from the records (zlib_from_blocks)              %10.1f   %s\n", t_blocks, ok3 ? "equal" : "DIFFERS");
    printf("tables, headers, offsets alone (BlockPlanner: form 3)   %10.1f   %.1f us a block\n", now_ms() - t0, 1e3 * (now_ms() - t0) / (double)nb);
  }
  t0 = now_ms();
  uint32_t s1 = 1, s2 = 0;
  for (size_t i = 0; i < n;) { const size_t blk = std::min<size_t>(5552, n - i); for (size_t j = 0; j < blk; j++) { s1 += x[i + j]; s2 += s1; } s1 %= 65521; s2 %= 65521; i += blk; }
  const double t_adler = now_ms() - t0;
  printf("Adler-32 alone (inside both of the above)               %10.1f   %08x\n", t_adler, (s2 << 16) | s1);
  printf("=> of zlib_from_matches: table look-ups and the parser's steps %.0f %%, token bookkeeping + block decisions + Huffman coding + bit output %.0f %%, Adler-32 %.0f %%\n",
         100 * (t_matches - t_tokens) / t_matches, 100 * (t_tokens - t_adler) / t_matches, 100 * t_adler / t_matches);
  return ok1 && ok2 ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "check")) return check();
  if (argc >= 3 && !strcmp(argv[1], "time")) return time_phases((size_t)atoi(argv[2]));
  fprintf(stderr, "usage: %s check | time LOG2\n", argv[0]);
  return 2;
}
