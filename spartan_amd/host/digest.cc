// spartan_amd host driver: R1CSShape::get_digest (src/r1cs.rs:154-158) with the device's help (option digest.device = 1, 2 or 3).
//   device   bincode(shape) serialised from the resident entries (sp_sparse_bincode); tdefl's match search, one input position per lane,
//            segment by segment (sp_deflate_*: csrc/deflate_match.hip); with digest.device = 2 the lazy parse as well (sp_deflate_open_parse:
//            walks between the parser's free states from the positions reachable from each segment's entry)
//   host     what is sequential (deflate.cc). digest.device = 1: the parser over the match tables L, A, B with the coder behind it
//            (MatchParser). digest.device = 2: the coder alone over the tokens the device hands over (TokenCoder: record_literal,
//            record_match, the block check and flush_block, no table look-up); L, A and B are then not downloaded. digest.device = 3: the
//            coder's block boundaries, histograms, bit emission, stored-block copies and Adler-32 on the device as well (sp_deflate_open_emit:
//            csrc/deflate_emit.hip); here only what is a function of a block's 320 counters and of the block before it (BlockPlanner: the
//            Huffman tables and the header, the stored-or-coded decision, the bit offsets) and the stitching of head and trailer. Neither
//            tokens nor input bytes come down: records and histograms do, tables and offsets go up, the compressed bytes come down once.
// All forms run one pipeline (run_segments): segment s is consumed here while the device works on segment s + 1; what the device made
// arrives through its two pinned slots. They differ in the wait call and in what consumes the segment.
// The bytes are those of zlib_level6_miniz by construction (tests/test_deflate_matches.py, tests/test_gpu_deflate_matches.py,
// tests/test_gpu_deflate_tokens.py). The Rust crate computes its digest with flate2 itself and has no use for this file, which is why it
// stands apart from prover.cc.
#include <chrono>

#include <hip/hip_runtime_api.h>

#include "libspartan.hpp"

namespace spz {
namespace {
double now_ms() { return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// an sp_* call: timed for host.callstats, its failure thrown
#define DSPX(call)                                                                                                                \
  do {                                                                                                                            \
    const double t0_ = now_ms();                                                                                                  \
    const int32_t rc_ = (call);                                                                                                   \
    std::string k_(#call);                                                                                                        \
    callstats_add(k_.substr(0, k_.find('(')).c_str(), (now_ms() - t0_) * 1e-3);                                                    \
    if (rc_ != SP_OK) throw Error(std::string(#call) + " failed: " + sp_strerror(rc_) + " (" + std::to_string(rc_) + ")");          \
  } while (0)
struct DeflateHandle {
  sp_deflate* d = nullptr;
  ~DeflateHandle() { sp_deflate_close(d); }
};
struct DeviceBytes {
  uint8_t* p = nullptr;
  ~DeviceBytes() { if (p) (void)hipFree(p); }
};
size_t log_2(size_t n) { size_t l = 0; while (((size_t)1 << l) < n) l++; return l; }

struct Arrived { size_t first = 0, count = 0; const uint8_t* bytes = nullptr; };  // a segment in its pinned slot: positions, and its bytes + 258
// The segment pipeline of both forms: segment s + 1 is started on the device before segment s is waited for, so the device works on it
// while the host consumes segment s. wait(s, a, ms) is the form's sp_deflate_segment_wait*; consume(D, bytes_end, a) hands what it left to the
// form's parser or coder, D[0, bytes_end) being the input as the host reads it (Adler-32, stored blocks, a fallback search): the caller's
// bytes, or the device's as they arrive (a match of this segment's tokens ends within 258 of its end); finish() returns the stream.
// stage[] sums the device's stage times in the form's order. bytes_arrive = false: the form reads no input byte here (D is then `data`, maybe null).
template <typename Wait, typename Consume, typename Finish>
std::vector<uint8_t> run_segments(sp_deflate* d, const uint8_t* data, size_t n, DeflateStats& S, double stage[6], Wait wait, Consume consume, Finish finish,
                                  bool bytes_arrive = true) {
  const size_t nseg = sp_deflate_segments(d);
  S.segments = (double)nseg;
  std::vector<uint8_t> arrived;
  if (!data && bytes_arrive) arrived.resize(n);
  if (nseg) DSPX(sp_deflate_segment_start(d, 0));
  for (size_t s = 0; s < nseg; s++) {
    if (s + 1 < nseg) DSPX(sp_deflate_segment_start(d, s + 1));
    Arrived a;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    const double t0 = now_ms();
    wait(s, a, ms);
    const double t1 = now_ms();
    S.ms_wait += t1 - t0;
    for (int i = 0; i < 6; i++) stage[i] += ms[i];
    const size_t have = std::min(n, a.first + a.count + 258);
    if (!data && bytes_arrive) memcpy(arrived.data() + a.first, a.bytes, have - a.first);
    consume(data || !bytes_arrive ? data : arrived.data(), data ? n : have, a);
    S.ms_parse += now_ms() - t1;
  }
  const double t2 = now_ms();
  std::vector<uint8_t> z = finish();
  S.ms_parse += now_ms() - t2;
  return z;
}

// bincode(R1CSShape) in device memory: the 24-byte header from here, the three matrices serialised where they live. Returns its length.
size_t shape_bincode_on_device(const Instance& I, DeviceBytes& buf, const std::string& who) {
  const size_t n = 24 + 3 * 24 + 48 * (I.nnz[0] + I.nnz[1] + I.nnz[2]);
  if (hipSetDevice(sp_ctx_device(I.c)) != hipSuccess) throw Error(who + ": hipSetDevice failed");
  if (hipMalloc((void**)&buf.p, n) != hipSuccess) throw Error(who + ": no device memory for bincode(shape)");
  const uint64_t head[3] = {I.num_cons, I.num_vars, I.num_inputs};
  if (hipMemcpy(buf.p, head, 24, hipMemcpyHostToDevice) != hipSuccess) throw Error(who + ": copy failed");
  const sp_sparse* ms[3] = {I.dA, I.dB, I.dC};
  DSPX(sp_sparse_bincode(I.c, ms, 3, log_2(I.num_cons), log_2(2 * I.num_vars), buf.p + 24, n - 24));
  return n;
}
}  // namespace

std::vector<uint8_t> zlib_device(sp_ctx* c, const uint8_t* data, const uint8_t* dev_data, size_t n, unsigned probes, bool old_header, DeflateStats* st,
                                 int parse, size_t tile, size_t group, size_t chunk) {
  DeflateStats own;
  DeflateStats& S = st ? *st : own;
  const double t_begin = now_ms();
  S.device = 1;
  if (hipSetDevice(sp_ctx_device(c)) != hipSuccess) throw Error("zlib_device: hipSetDevice failed");
  if (parse < 0) parse = std::max(0, (int)ctx_opt(c, "digest.device") - 1);  // 1 -> the host parser, 2 -> the device parse, 3 -> the device coder
  if (parse > 2) throw Error("zlib_device: no such form");
  const uint8_t* src = dev_data ? dev_data : data;
  DeflateHandle h;
  double stage[6] = {0, 0, 0, 0, 0, 0};
  std::vector<uint8_t> z;
  if (parse == 2) {  // the device hands over block records and takes tables and offsets; the compressed bytes come down at the end
    DSPX(sp_deflate_open_emit(c, src, n, dev_data != nullptr, probes, tile, group, chunk, &h.d));
    BlockPlanner planner(probes, old_header);
    size_t nb = 0;
    const uint64_t* rec = nullptr;
    const uint16_t* hist = nullptr;
    uint64_t adler[2] = {0, 0}, carry[4] = {0, 0, 0, 0};
    uint32_t s1 = 1, s2 = 0;
    std::vector<uint64_t> plans;
    std::vector<uint32_t> tables;
    std::vector<uint8_t> hdrs;
    BlockPlan p;
    auto plan_blocks = [&](size_t count) {  // tables, header, decision and offset of every block just closed
      const double t0 = now_ms();
      plans.resize(6 * nb); tables.resize(BLOCK_HIST * nb); hdrs.resize(BLOCK_HDR_BYTES * nb);
      for (size_t b = 0; b < nb; b++) {
        planner.plan(rec + BLOCK_REC * b, hist + BLOCK_HIST * b, p);
        uint64_t* q = plans.data() + 6 * b;
        q[0] = p.bit_off; q[1] = p.hdr_bits; q[2] = p.kind; q[3] = p.tok_off; q[4] = p.eob_off; q[5] = p.src;
        memcpy(tables.data() + BLOCK_HIST * b, p.table, sizeof p.table);
        memcpy(hdrs.data() + BLOCK_HDR_BYTES * b, p.hdr, sizeof p.hdr);
        S.tokens_coded += (double)rec[BLOCK_REC * b + 1];
      }
      s2 = (uint32_t)((s2 + (uint64_t)(count % 65521) * s1 + adler[1]) % 65521);  // Adler-32 over the segment from its pair
      s1 = (uint32_t)((s1 + adler[0]) % 65521);
      S.ms_tables += now_ms() - t0;
    };
    size_t seg = 0;
    z = run_segments(
        h.d, data, n, S, stage,
        [&](size_t s, Arrived& a, double* ms) {
          seg = s;
          DSPX(sp_deflate_segment_wait_blocks(h.d, s, &a.first, &a.count, &nb, &rec, &hist, adler, carry, ms));
        },
        [&](const uint8_t*, size_t, const Arrived& a) {
          S.device_fallbacks = (double)carry[3];
          plan_blocks(a.count);
          DSPX(sp_deflate_segment_emit(h.d, seg, nb, plans.data(), tables.data(), hdrs.data()));
        },
        [&] {
          if (!n) {  // no segment: the one block is the empty finish block, all of it written here
            const uint64_t r[BLOCK_REC] = {0, 0, 0, tdefl::RULE_FINISH, 0, 0};
            const uint16_t none[BLOCK_HIST] = {0};
            uint64_t st3[3];
            std::vector<uint8_t> e = zlib_from_blocks(r, none, 1, nullptr, nullptr, 0, probes, old_header, st3);
            S.blocks = 1; S.static_blocks = 1;
            return e;
          }
          const double t0 = now_ms();
          std::vector<uint8_t> out(planner.stream_bytes(), 0);
          double ms_bits = 0;
          DSPX(sp_deflate_emit_bytes(h.d, out.data(), out.size() - 4, &ms_bits));
          planner.finish(out, (s2 << 16) | s1);
          S.ms_bits += ms_bits; S.ms_bytes += now_ms() - t0;
          S.blocks = (double)planner.blocks; S.stored_blocks = (double)planner.stored_blocks; S.static_blocks = (double)planner.static_blocks;
          return out;
        },
        false);
    S.parse = 1; S.emit = 1;
    S.ms_reach += stage[3]; S.ms_emit += stage[4]; S.ms_blocks += stage[5];
  } else if (parse) {  // the device hands over tokens; the coder behind it
    DSPX(sp_deflate_open_parse(c, src, n, dev_data != nullptr, probes, tile, group, &h.d));
    TokenCoder coder(n, probes, old_header);
    const uint32_t* tokens = nullptr;
    size_t ntok = 0;
    uint64_t carry[4] = {0, 0, 0, 0};
    z = run_segments(
        h.d, data, n, S, stage,
        [&](size_t s, Arrived& a, double* ms) { DSPX(sp_deflate_segment_wait_tokens(h.d, s, &a.first, &a.count, &a.bytes, &tokens, &ntok, carry, ms)); },
        [&](const uint8_t* D, size_t bytes_end, const Arrived&) {
          S.tokens += (double)ntok; S.device_fallbacks = (double)carry[3];
          coder.code(D, bytes_end, tokens, ntok);
        },
        [&] { return coder.finish(); });
    S.parse = 1;
    S.ms_reach += stage[3]; S.ms_emit += stage[4]; S.ms_download += stage[5];
  } else {  // the device hands over the tables L, A, B; the parser over them, and the coder behind it
    DSPX(sp_deflate_open(c, src, n, dev_data != nullptr, probes, &h.d));
    MatchParser parser(n, probes, old_header);
    const uint16_t* L = nullptr;
    const uint32_t *A = nullptr, *B = nullptr;
    z = run_segments(
        h.d, data, n, S, stage,
        [&](size_t s, Arrived& a, double* ms) { DSPX(sp_deflate_segment_wait(h.d, s, &a.first, &a.count, &a.bytes, &L, &A, &B, ms)); },
        [&](const uint8_t* D, size_t, const Arrived& a) { parser.parse(D, a.first, a.count, L, A, B); },
        [&] { return parser.finish(); });
    S.lookups = (double)parser.lookups; S.fallbacks = (double)parser.fallbacks;
    S.ms_download += stage[3];
  }
  S.ms_links += stage[0]; S.ms_search_a += stage[1]; S.ms_search_b += stage[2];
  S.ms_total += now_ms() - t_begin;
  return z;
}

// the digest from bincode(R1CSShape) in device memory
std::vector<uint8_t> Instance::compute_digest_device() const {
  DeflateStats S;
  const double t0 = now_ms();
  DeviceBytes buf;
  const size_t n = shape_bincode_on_device(*this, buf, "Instance::compute_digest");
  S.ms_stream = now_ms() - t0;
  std::vector<uint8_t> z = zlib_device(c, nullptr, buf.p, n, 128, digest_old_header, &S);
  S.ms_total = now_ms() - t0;
  digest_stats = S;
  return z;
}
std::vector<uint8_t> Instance::shape_bincode_device() const {
  DeviceBytes buf;
  std::vector<uint8_t> b(shape_bincode_on_device(*this, buf, "Instance::shape_bincode_device"));
  if (hipMemcpy(b.data(), buf.p, b.size(), hipMemcpyDeviceToHost) != hipSuccess) throw Error("Instance::shape_bincode_device: copy failed");
  return b;
}
}  // namespace spz
