// spartan_amd host driver: R1CSShape::get_digest (src/r1cs.rs:154-158) with the device's help (option digest.device = 1).
//   device   bincode(shape) serialised from the resident entries (sp_sparse_bincode); tdefl's match search, one input position per lane,
//            segment by segment (sp_deflate_*: csrc/deflate_match.hip)
//   host     the parser over the match tables, the block decisions, the Huffman coding and the bit output (deflate.cc, MatchParser): all of
//            it sequential, all of it here. Segment s is parsed while the device searches segment s + 1; tables and bytes arrive through
//            the search's two pinned slots.
// With digest.device = 2 the lazy parse runs on the device as well (sp_deflate_open_parse: walks between the parser's free states from the
// positions reachable from each segment's entry) and the host codes the tokens it hands over (deflate.cc, TokenCoder): record_literal,
// record_match, the block check and flush_block, no table look-up. L, A and B are then not downloaded.
// The bytes are those of zlib_level6_miniz by construction (tests/test_deflate_matches.py, tests/test_gpu_deflate_matches.py). The Rust
// crate computes its digest with flate2 itself and has no use for this file, which is why it stands apart from prover.cc.
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
// the device parse and the token coder: segment s + 1 is searched and parsed on the device while the tokens of segment s are coded here
std::vector<uint8_t> zlib_device_tokens(sp_ctx* c, const uint8_t* data, const uint8_t* dev_data, size_t n, unsigned probes, bool old_header, DeflateStats& S,
                                        size_t tile, size_t group) {
  DeflateHandle h;
  DSPX(sp_deflate_open_parse(c, dev_data ? dev_data : data, n, dev_data != nullptr, probes, tile, group, &h.d));
  const size_t nseg = sp_deflate_segments(h.d);
  S.segments = (double)nseg;
  S.parse = 1;
  TokenCoder coder(n, probes, old_header);
  std::vector<uint8_t> arrived;  // the input as the coder reads it (Adler-32, stored blocks): the caller's bytes, or the device's as they arrive
  if (!data) arrived.resize(n);
  if (nseg) DSPX(sp_deflate_segment_start(h.d, 0));
  for (size_t s = 0; s < nseg; s++) {
    if (s + 1 < nseg) DSPX(sp_deflate_segment_start(h.d, s + 1));
    size_t first = 0, count = 0, ntok = 0;
    const uint8_t* bytes; const uint32_t* tokens;
    uint64_t carry[4];
    double ms[6];
    const double t0 = now_ms();
    DSPX(sp_deflate_segment_wait_tokens(h.d, s, &first, &count, &bytes, &tokens, &ntok, carry, ms));
    const double t1 = now_ms();
    S.ms_wait += t1 - t0;
    S.ms_links += ms[0]; S.ms_search_a += ms[1]; S.ms_search_b += ms[2]; S.ms_reach += ms[3]; S.ms_emit += ms[4]; S.ms_download += ms[5];
    S.tokens += (double)ntok; S.device_fallbacks = (double)carry[3];
    if (!data) memcpy(arrived.data() + first, bytes, std::min(n - first, count + 258));  // a match of this segment's tokens ends within 258 of its end
    coder.code(data ? data : arrived.data(), data ? n : std::min(n, first + count + 258), tokens, ntok);
    S.ms_parse += now_ms() - t1;
  }
  const double t2 = now_ms();
  std::vector<uint8_t> z = coder.finish();
  S.ms_parse += now_ms() - t2;
  return z;
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
  if (parse) {
    std::vector<uint8_t> z = zlib_device_tokens(c, data, dev_data, n, probes, old_header, S, tile, group);
    S.ms_total += now_ms() - t_begin;
    return z;
  }
  DeflateHandle h;
  DSPX(sp_deflate_open(c, dev_data ? dev_data : data, n, dev_data != nullptr, probes, &h.d));
  const size_t nseg = sp_deflate_segments(h.d);
  S.segments = (double)nseg;
  MatchParser parser(n, probes, old_header);
  // the input as the parser reads it: the caller's bytes, or the device's as they arrive with each segment
  std::vector<uint8_t> arrived;
  if (!data) arrived.resize(n);
  if (nseg) DSPX(sp_deflate_segment_start(h.d, 0));
  for (size_t s = 0; s < nseg; s++) {
    if (s + 1 < nseg) DSPX(sp_deflate_segment_start(h.d, s + 1));  // searched while segment s is parsed
    size_t first = 0, count = 0;
    const uint8_t* bytes; const uint16_t* L; const uint32_t *A, *B;
    double ms[4];
    const double t0 = now_ms();
    DSPX(sp_deflate_segment_wait(h.d, s, &first, &count, &bytes, &L, &A, &B, ms));
    const double t1 = now_ms();
    S.ms_wait += t1 - t0;
    S.ms_links += ms[0]; S.ms_search_a += ms[1]; S.ms_search_b += ms[2]; S.ms_download += ms[3];
    if (!data) {
      const size_t have = std::min(n - first, count + 258);
      memcpy(arrived.data() + first, bytes, have);
    }
    parser.parse(data ? data : arrived.data(), first, count, L, A, B);
    S.ms_parse += now_ms() - t1;
  }
  const double t2 = now_ms();
  std::vector<uint8_t> z = parser.finish();
  S.ms_parse += now_ms() - t2;
  S.lookups = (double)parser.lookups; S.fallbacks = (double)parser.fallbacks;
  S.ms_total += now_ms() - t_begin;
  return z;
}

// bincode(R1CSShape) in device memory, the three matrices serialised where they live; the digest from there
std::vector<uint8_t> Instance::compute_digest_device() const {
  DeflateStats S;
  const double t0 = now_ms();
  const size_t n = 24 + 3 * 24 + 48 * (nnz[0] + nnz[1] + nnz[2]);
  DeviceBytes buf;
  if (hipSetDevice(sp_ctx_device(c)) != hipSuccess) throw Error("Instance::compute_digest: hipSetDevice failed");
  if (hipMalloc((void**)&buf.p, n) != hipSuccess) throw Error("Instance::compute_digest: no device memory for bincode(shape)");
  const uint64_t head[3] = {num_cons, num_vars, num_inputs};
  if (hipMemcpy(buf.p, head, 24, hipMemcpyHostToDevice) != hipSuccess) throw Error("Instance::compute_digest: copy failed");
  const sp_sparse* ms[3] = {dA, dB, dC};
  DSPX(sp_sparse_bincode(c, ms, 3, log_2(num_cons), log_2(2 * num_vars), buf.p + 24, n - 24));
  S.ms_stream = now_ms() - t0;
  std::vector<uint8_t> z = zlib_device(c, nullptr, buf.p, n, 128, digest_old_header, &S);
  S.ms_total = now_ms() - t0;
  digest_stats = S;
  return z;
}
std::vector<uint8_t> Instance::shape_bincode_device() const {
  const size_t n = 24 + 3 * 24 + 48 * (nnz[0] + nnz[1] + nnz[2]);
  DeviceBytes buf;
  if (hipSetDevice(sp_ctx_device(c)) != hipSuccess) throw Error("Instance::shape_bincode_device: hipSetDevice failed");
  if (hipMalloc((void**)&buf.p, n) != hipSuccess) throw Error("Instance::shape_bincode_device: no device memory");
  const sp_sparse* ms[3] = {dA, dB, dC};
  DSPX(sp_sparse_bincode(c, ms, 3, log_2(num_cons), log_2(2 * num_vars), buf.p + 24, n - 24));
  std::vector<uint8_t> b(n);
  const uint64_t head[3] = {num_cons, num_vars, num_inputs};
  memcpy(b.data(), head, 24);
  if (hipMemcpy(b.data() + 24, buf.p + 24, n - 24, hipMemcpyDeviceToHost) != hipSuccess) throw Error("Instance::shape_bincode_device: copy failed");
  return b;
}
}  // namespace spz
