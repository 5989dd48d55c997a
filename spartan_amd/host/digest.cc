// spartan_amd host driver: R1CSShape::get_digest (src/r1cs.rs:154-158) with the device's help (option digest.device = 1 or 2).
//   device   bincode(shape) serialised from the resident entries (sp_sparse_bincode); tdefl's match search, one input position per lane,
//            segment by segment (sp_deflate_*: csrc/deflate_match.hip); with digest.device = 2 the lazy parse as well (sp_deflate_open_parse:
//            walks between the parser's free states from the positions reachable from each segment's entry)
//   host     what is sequential (deflate.cc). digest.device = 1: the parser over the match tables L, A, B with the coder behind it
//            (MatchParser). digest.device = 2: the coder alone over the tokens the device hands over (TokenCoder: record_literal,
//            record_match, the block check and flush_block, no table look-up); L, A and B are then not downloaded.
// Both forms run one pipeline (run_segments): segment s is consumed here while the device works on segment s + 1; what the device made
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
// stage[] sums the device's stage times in the form's order.
template <typename Wait, typename Consume, typename Finish>
std::vector<uint8_t> run_segments(sp_deflate* d, const uint8_t* data, size_t n, DeflateStats& S, double stage[6], Wait wait, Consume consume, Finish finish) {
  const size_t nseg = sp_deflate_segments(d);
  S.segments = (double)nseg;
  std::vector<uint8_t> arrived;
  if (!data) arrived.resize(n);
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
    if (!data) memcpy(arrived.data() + a.first, a.bytes, have - a.first);
    consume(data ? data : arrived.data(), data ? n : have, a);
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
                                 int parse, size_t tile, size_t group) {
  DeflateStats own;
  DeflateStats& S = st ? *st : own;
  const double t_begin = now_ms();
  S.device = 1;
  if (hipSetDevice(sp_ctx_device(c)) != hipSuccess) throw Error("zlib_device: hipSetDevice failed");
  if (parse < 0) parse = ctx_opt(c, "digest.device") == 2;
  const uint8_t* src = dev_data ? dev_data : data;
  DeflateHandle h;
  double stage[6] = {0, 0, 0, 0, 0, 0};
  std::vector<uint8_t> z;
  if (parse) {  // the device hands over tokens; the coder behind it
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
