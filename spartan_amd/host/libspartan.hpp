// spartan_amd host driver: C++ mirror of libspartan's public API (src/lib.rs) for the prover path, on top of
// the C ABI in include/spartan_hip.h. It exists because no Rust toolchain is available here; in the drop-in
// deployment this layer IS libspartan (Rust) with the `gpu` feature. Names and argument
// meaning follow the reference: Instance, VarsAssignment/InputsAssignment, SNARKGens, NIZKGens,
// ComputationCommitment/Decommitment, SNARK::{encode,prove,verify}, NIZK::{prove,verify} (the verifiers: verifier.cc).
//
// All table-sized field/group work of the prover runs on the GPU through sp_* calls; the host keeps what the
// reference keeps next to its Transcript — Fiat–Shamir, O(log n)-sized scalar bookkeeping, serialization — and the
// 2..5-term commitments of the Sigma protocols, whose dependent chains a host core finishes before a lone wavefront
// would (the library's host-side engine, sp_host_*).
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/spartan_host.h"  // the driver's C boundary; brings spartan_hip.h
#include "transcript.hpp"
#include "../csrc/tdefl_rules.hpp"  // the token word (TOK_*) and the rules behind the deflate declarations below

namespace spz {

typedef std::array<uint8_t, 32> CP;  // CompressedGroup (src/group.rs:7)
typedef std::vector<Fq> FqVec;

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// value of a library option of the context (spartan_amd/csrc/options.hpp; sp_ctx_set_option): the driver's own switches live in the same table
inline long long ctx_opt(const sp_ctx* c, const char* key) {
  int64_t v = 0;
  if (sp_ctx_get_option(c, key, &v) != SP_OK) throw std::runtime_error(std::string("unknown library option ") + key);
  return (long long)v;
}

// ---- device handles (RAII) ----
struct Ctx {
  sp_ctx* h = nullptr;
  explicit Ctx(int device);
  ~Ctx();
  Ctx(const Ctx&) = delete;
};
// Row-sharded DensePolynomial::commit across the GPUs of one node (spartan_amd/host/shard.cc): every rank
// runs the same proof in lock-step; for a commitment of L rows rank r computes rows [r L/W, (r+1) L/W) and the 32-byte
// compressed commitments are exchanged with one all-gather of bytes (rows are independent MSMs: no elliptic-curve
// reduction exists in RCCL and none is needed). Three transports:
//   set_commit_shard_rccl     RCCL inside the library: rank 0 draws the id (rccl_unique_id), the caller hands it to every
//                             rank by whatever channel it has, each rank joins with ncclCommInitRank; commits then use
//                             ncclAllGather on device buffers. librccl.so is dlopen'ed on first use.
//   set_commit_shard          the caller moves the bytes: gather(user, buf, total, off, len) — on entry buf[off, off+len)
//                             holds this rank's bytes, on return buf[0, total) is complete (tests: gloo)
//   set_commit_shard_virtual  W shards on ONE GPU (W sub-contexts, in-process gather): the partitioning under test
// world <= 1 (or nshards <= 1) clears the setting. All ranks must then run identical prove() calls.
// CONTRACT OF THE TWO MULTI-PROCESS TRANSPORTS: configuring the sharding is itself a collective — set_commit_shard / set_commit_shard_rccl
// exchange 8 bytes per rank over the transport they were just given (check_switches_agree, shard.cc: ranks whose sharding options differ
// fail there with a message instead of deadlocking in the first proof). Every rank must therefore call it at the same point, and the
// gather callback must already work when it is handed over.
void unipoly_probe(const FqVec& evals, const Fq& r, FqVec* coeffs, FqVec* compressed, Fq* eval_at_r);  // test hook
void cubic_coeffs_probe(const Fq S[12], const Fq& r, Fq ev[3]);                                                // test hook (spark.inc)
void cubic_tail_probe(FqVec& tab, size_t ni, size_t m, const FqVec& coeffs, const FqVec& challenges, FqVec* evs);  // test hook (spark.inc)
bool eq_factor_probe(const FqVec& rho, size_t np, size_t ni, const FqVec& coeffs, const FqVec& claims, const FqVec& ev4, const FqVec& challenges, FqVec* evc_out,
                     FqVec* K_out);  // test hook (spark.inc)
typedef spz_commit_gather_fn CommitGatherFn;  // spartan_host.h
void set_commit_shard(Ctx& c, int rank, int world, CommitGatherFn gather, void* user);
void rccl_unique_id(uint8_t out[128]);
void set_commit_shard_rccl(Ctx& c, int rank, int world, const uint8_t unique_id[128]);
void set_commit_shard_virtual(Ctx& c, int nshards);
struct ShardStats { size_t gathers = 0, bytes = 0; };  // exchanges since the last reset (bench.py reports them per proof)
ShardStats commit_shard_stats(Ctx& c, bool reset);
// internal to the driver (prover.cc <-> shard.cc)
bool commit_shard_active(sp_ctx* c);
std::vector<sp_ctx*> residue_shard_ctxs(sp_ctx* c);  // virtual shards: [c, sub-contexts...]; empty when none
void commit_shard_note_gather(sp_ctx* c, size_t bytes);
// callback / RCCL transport configured: this rank's place among the lock-step ranks, and the table length (log2) from which a sum-check is
// residue-sharded over it (resolved once when the sharding was configured, identical on every rank: shard.cc, check_switches_agree)
bool commit_shard_transport(sp_ctx* c, int* rank, int* world, int* residue_min_log2 = nullptr);
bool commit_shard_residue_off(sp_ctx* c);  // option shard.residues = 0 as resolved when the sharding was configured
void commit_shard_gather(sp_ctx* c, uint8_t* all, size_t per);   // all-gather of `per` bytes per rank over that transport (rank order)
double rccl_allgather_probe(sp_ctx* c, size_t bytes, int iters);  // us per H2D + ncclAllGather + D2H + sync of `bytes` per rank
bool commit_shard_shared_seed(sp_ctx* c, Fq* seed);  // multi-rank transports only: a hash of every rank's OS-entropy contribution, the same on every rank
void commit_shard_forget(sp_ctx* c);
bool sharded_commit_rows(sp_ctx* c, const sp_gens* g, size_t g_off, size_t h_idx, const sp_table* Z, size_t Ls, size_t Rs, const uint64_t* blinds,
                         uint8_t* out);
struct DevTable {  // DensePolynomial with Z resident in HBM (src/dense_mlpoly.rs:14-18)
  sp_ctx* c = nullptr;
  sp_table* h = nullptr;
  DevTable() {}
  DevTable(sp_ctx* c_, sp_table* h_) : c(c_), h(h_) {}
  DevTable(DevTable&& o) noexcept : c(o.c), h(o.h) { o.h = nullptr; }
  DevTable& operator=(DevTable&& o) noexcept;
  DevTable(const DevTable&) = delete;
  ~DevTable();
  size_t len() const { return sp_table_len(h); }
};

// MultiCommitGens (src/commitments.rs:8-13) as a view into a device generator stream
struct MultiCommitGens {
  sp_gens* g = nullptr;           // the stream's fixed-base set; null under verifier-only generators
  const sp_points* p = nullptr;   // ... whose stream is a resident point set instead (GensStream::pts)
  std::vector<uint32_t> G;  // stream indices of G[0..n)
  uint32_t h = 0;           // stream index of h
  size_t n() const { return G.size(); }
};
struct DotProductProofGens {  // src/nizk/mod.rs:408-419
  size_t n;
  MultiCommitGens gens_n, gens_1;
};
struct PolyCommitmentGens {  // src/dense_mlpoly.rs:25-36
  DotProductProofGens gens;
};
// One SHAKE256 stream of points (label). The prover's form is uploaded once with its fixed-base window tables (g). The VERIFIER-ONLY form
// (verifier_only, verifier.cc) has the same points, the same `compressed` bytes and the same index structure, but no sp_gens: the stream is a
// resident point set (pts: 64 KiB a point, made on the device from the same uniform bytes), which is all a verification multiplies over.
struct GensStream {
  sp_ctx* c = nullptr;
  sp_gens* g = nullptr;
  std::shared_ptr<sp_points> pts;  // verifier-only form; freed by the deleter verifier.cc gave it
  std::vector<uint8_t> compressed;
  GensStream() {}
  GensStream(sp_ctx* c, const char* label, size_t npoints, int windows = 0 /* table geometry planned by the caller, or 0: the library's per-set policy */);
  GensStream(GensStream&& o) noexcept : c(o.c), g(o.g), pts(std::move(o.pts)), compressed(std::move(o.compressed)) { o.g = nullptr; }
  GensStream& operator=(GensStream&& o) noexcept;
  ~GensStream();
  static std::vector<uint8_t> uniform_bytes(const char* label, size_t npoints);  // 64 bytes a point: SHAKE256(label || basepoint) (commitments.rs:16-19)
  static GensStream verifier_only(sp_ctx* c, const char* label, size_t npoints);  // verifier.cc
  size_t npoints() const { return compressed.size() / 32; }
  MultiCommitGens multi_commit_gens(size_t n) const;        // MultiCommitGens::new(n, label)
  DotProductProofGens dot_product_gens(size_t n) const;     // DotProductProofGens::new(n, label)
  PolyCommitmentGens poly_commitment_gens(size_t num_vars) const;
};
struct R1CSSumcheckGens { MultiCommitGens gens_1, gens_3, gens_4; };  // src/r1csproof.rs:39-60
struct R1CSGens {                                                      // src/r1csproof.rs:62-74
  R1CSSumcheckGens gens_sc;
  PolyCommitmentGens gens_pc;
};
struct SparseMatPolyCommitmentGens { PolyCommitmentGens gens_ops, gens_mem, gens_derefs; };  // src/sparse_mlpoly.rs:302-337

// Point counts and polynomial sizes of the generator streams of an instance shape (lib.rs:288-307, 476-484): shared by the prover's
// constructors and the verifier-only ones, which differ only in how a stream is made.
struct GensLayout {
  size_t num_vars_padded = 0, sat_points = 0;                                   // gens_r1cs_sat
  size_t num_vars_ops = 0, num_vars_mem = 0, num_vars_derefs = 0, eval_points = 0;  // gens_r1cs_eval (SNARK only)
  size_t num_nz_padded = 0;
  GensLayout(size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries);
};
struct NIZKGens {  // src/lib.rs:468-486
  GensStream stream_sat;
  R1CSGens gens_r1cs_sat;
  NIZKGens(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs);
  // the verifier's form (verifier.cc): NIZK::verify / verify_many take it; NIZK::prove refuses it
  static NIZKGens verifier_only(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs);
  bool is_verifier_only() const { return stream_sat.g == nullptr; }
  size_t resident_bytes() const;  // HBM held by the stream's tables, either form
 private:
  NIZKGens() {}
  void index(const GensLayout& l);  // the MultiCommitGens views into the stream
};
struct SNARKGens {  // src/lib.rs:276-309
  GensStream stream_sat, stream_eval;
  R1CSGens gens_r1cs_sat;
  SparseMatPolyCommitmentGens gens_r1cs_eval;
  SNARKGens(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries);
  // the verifier's form (verifier.cc): SNARK::verify / verify_many take it; SNARK::encode and SNARK::prove refuse it
  static SNARKGens verifier_only(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries);
  bool is_verifier_only() const { return stream_sat.g == nullptr; }
  size_t resident_bytes() const;  // HBM held by the two streams' tables, either form
  // bincode of the serde-derived struct (lib.rs:278-282 -> r1csproof.rs:39-66, r1cs.rs:28-31, sparse_mlpoly.rs:284-289,
  // dense_mlpoly.rs:24-27, nizk/mod.rs:407-412, commitments.rs:7-12): every MultiCommitGens is {n, Vec<G>, h}, points as 32 bytes
  std::vector<uint8_t> serialize() const;
 private:
  SNARKGens() {}
  void index(const GensLayout& l);  // the MultiCommitGens views into the two streams
};

// Figures of one device-assisted deflate (digest.cc), as spz_zlib_device and spz_instance_digest_stats report them
struct DeflateStats {
  double lookups = 0, fallbacks = 0, segments = 0;
  double ms_links = 0, ms_search_a = 0, ms_search_b = 0, ms_download = 0;  // device time, from events on the search's stream
  double ms_parse = 0, ms_wait = 0, ms_stream = 0, ms_total = 0;            // host wall time: parse + coding, waiting for the device, building the stream
  double device = 0;                                                        // 1: the device-assisted path ran
  // the device parse (digest.device = 2): 1 when it ran, tokens it handed over, look-ups it searched on the spot (those neither table answers),
  // device time of the reachability kernels (jumps, exits, composition, entries, marks) and of the token kernel with its compaction.
  // ms_parse is then the token coder alone, ms_download the copies of tokens and bytes, lookups / fallbacks stay 0 (nothing is looked up here)
  double parse = 0, tokens = 0, device_fallbacks = 0, ms_reach = 0, ms_emit = 0;
  // the device coder (digest.device = 3): 1 when it ran; then `tokens` stays 0 (none is handed over) and tokens_coded counts them from the
  // block records; blocks, stored and static blocks among them; device time of the block stage (costs, scan, boundaries, histograms,
  // Adler-32, the records' copy) and of the bit emission; host time of the table building (within ms_parse) and of the one download of the
  // compressed bytes
  double emit = 0, tokens_coded = 0, blocks = 0, stored_blocks = 0, static_blocks = 0, ms_blocks = 0, ms_bits = 0, ms_tables = 0, ms_bytes = 0;
};

// ---- instance ----
struct SparseEntry { uint64_t row, col; Fq val; };
struct VarsAssignment;
// What Instance::is_sat found: the number of constraints with (A z)[r] * (B z)[r] != (C z)[r], the smallest such r (UINT64_MAX when there is
// none) and the lowest `max_rows` of them in ascending order — the caller's constraint numbers (Instance::new pads rows at the end only).
struct SatReport { uint64_t violated = 0, first_row = UINT64_MAX; std::vector<uint64_t> rows; };
struct Instance {  // src/lib.rs:110-273 (R1CSInstance after padding) with the matrices resident on the device
  sp_ctx* c = nullptr;
  size_t num_cons = 0, num_vars = 0, num_inputs = 0;
  std::vector<SparseEntry> A, B, C;  // the padded, shifted entries of an instance made on the host; empty for one made by from_entries
  size_t nnz[3] = {0, 0, 0};         // entries of A, B, C after padding, whichever way the instance was made
  bool resident_only = false;        // made by from_entries / from_device_entries: the entries live in dA, dB, dC alone
  sp_sparse *dA = nullptr, *dB = nullptr, *dC = nullptr;
  // R1CSShapeDigest bytes: zlib(level 6)(bincode(shape)) (r1cs.rs:154-158), absorbed by NIZK::prove (lib.rs:514). Computed on first
  // use by compute_digest() (deflate.cc: a restatement of miniz's level-6 tdefl, what flate2's rust_backend runs — byte-identical to the
  // real C miniz 3.0.2 on the test corpus); a caller that holds the bytes of a real libspartan Instance may set them instead
  // (set_digest). With the option digest.device = 1 (the default) the stream is serialised and the deflater's match search runs on the
  // device, and only its parser and Huffman coding run here (digest.cc; the same bytes; digest.device = 2: the lazy parse on the device
  // too, only the token coder here — 13 % faster at 2^20, not at 2^16: profiles/instance_digest_parse.txt; digest.device = 3: the coder on
  // the device too, only the Huffman tables and bit offsets here — 3.2x faster at both: profiles/instance_digest_emit.txt). The computation is guarded: concurrent
  // NIZK::prove calls over one Instance compute it once; a caller that wants the deflate of a large shape (4.5 s at 2^20 with 9.4 M
  // entries, 19.9 s on the host alone: profiles/instance_digest.txt) out of its first prove calls compute_digest() right after
  // construction, as the reference's Instance::new does (lib.rs:228).
  mutable std::vector<uint8_t> digest;
  bool digest_old_header = false;  // zlib header 0x78 0x01 (miniz < 2.2, miniz_oxide 0.3) instead of 0x78 0x9C; set before the first compute_digest()
  mutable std::mutex digest_mu;
  std::vector<uint8_t> shape_bincode() const;  // bincode(R1CSShape): r1cs.rs:18-26, sparse_mlpoly.rs:19-38
  std::vector<uint8_t> compute_digest() const;
  // option digest.device = 1 (digest.cc): the stream serialised and its matches searched on the device, parsed and coded here; the same bytes
  std::vector<uint8_t> compute_digest_device() const;
  std::vector<uint8_t> shape_bincode_device() const;  // test hook: bincode(shape) as sp_sparse_bincode writes it
  mutable DeflateStats digest_stats;                  // figures of the last computation (device == 0: the host path; only ms_total is set)
  bool set_digest_header(bool old_header);
  void set_digest(const uint8_t* d, size_t n);
  // Instance::new (lib.rs:121-228): padding of num_cons / num_vars and the column shift are applied here.
  Instance(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const std::vector<SparseEntry>& A,
           const std::vector<SparseEntry>& B, const std::vector<SparseEntry>& C);
  ~Instance();
  Instance(const Instance&) = delete;
  // Instance::new as the reference takes it, built on the device (sp_sparse_from_entries): the entries of A, B, C back to back, nnz[k] of
  // each; rows and cols as usize, vals as canonical little-endian scalars of 32 bytes. Only the indices and the bytes cross PCIe: index test,
  // comparison with q, Montgomery form, column shift, pad entries and the two sorted copies are made in HBM, and no host copy of the entries
  // is kept (shape_bincode downloads them when the digest is computed). Throws InvalidIndex / InvalidScalar for the first matrix that fails
  // and, within it, the lowest failing entry: where the reference's loops return.
  static std::unique_ptr<Instance> from_entries(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3],
                                                const uint64_t* rows, const uint64_t* cols, const uint8_t* vals);
  // The same from three entry lists in the memory of the context's device, each (rows, cols, vals) of its own and at any alignment: nothing
  // visits the host. The caller has completed the work that wrote them (sp_sparse_from_entries_dev).
  static std::unique_ptr<Instance> from_device_entries(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3],
                                                       const uint64_t* const rows[3], const uint64_t* const cols[3], const uint8_t* const vals[3]);
  // Instance::produce_synthetic_r1cs (lib.rs:262-273 -> r1cs.rs:160-238) with the OsRng replaced by a SHAKE256
  // stream keyed by `seed` ("spartan-synthetic-r1cs" || LE64(seed)); returns the satisfying assignment.
  static std::unique_ptr<Instance> produce_synthetic_r1cs(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, uint64_t seed,
                                                          FqVec* vars, FqVec* inputs);
  // Instance::is_sat (lib.rs:230-259 -> r1cs.rs:240-266) on the device (sp_r1cs_check): one round trip, nothing table-sized crosses PCIe.
  // Throws Error("InvalidNumberOfInputs") where the reference returns Err: more variables than the padded num_vars, or inputs.size() !=
  // num_inputs; fewer variables are zero-padded. prove() does not call it: a caller checks, then proves, on the same resident assignment.
  bool is_sat(const Fq* vars, size_t num_vars_given, const FqVec& inputs, SatReport* report = nullptr, size_t max_rows = 0,
              const sp_table* vars_resident = nullptr) const;
  bool is_sat(const VarsAssignment& vars, const FqVec& inputs, SatReport* report = nullptr, size_t max_rows = 0) const;
 private:
  explicit Instance(sp_ctx* ctx) : c(ctx) {}
  template <typename F>
  static std::unique_ptr<Instance> build_resident(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], F make);
};
// VarsAssignment (lib.rs:56-105, Assignment::new) with the scalars resident in HBM: the reference parses the caller's bytes
// into Scalars in the constructor, outside prove; here the constructor also uploads them, once, and every proof over the
// assignment starts from the device copy (one 32 MB PCIe transfer less per 2^20 proof). The padding to the instance's
// num_vars (lib.rs:360-368) stays in prove.
struct VarsAssignment {
  sp_ctx* c = nullptr;
  DevTable tab;
  size_t n = 0;
  VarsAssignment(Ctx& ctx, const Fq* vars, size_t n);
  // Assignment::new (lib.rs:62-88) as the reference takes it: n canonical little-endian scalars of 32 bytes. Only the bytes cross PCIe; they
  // are checked against q and brought into Montgomery form on the device (sp_table_from_bytes). A value >= q throws InvalidScalar, where the
  // reference returns R1CSError::InvalidScalar, and nothing stays allocated.
  static VarsAssignment from_bytes(Ctx& ctx, const uint8_t* bytes, size_t n);
  // The same from 32 n bytes in the memory of the context's device, at any alignment (a witness a kernel produced): they never visit the host.
  // The caller has completed the work that wrote them (sp_table_from_bytes_dev).
  static VarsAssignment from_device_bytes(Ctx& ctx, const uint8_t* dev, size_t n);
  std::vector<uint8_t> to_bytes() const;  // Scalar::to_bytes of every entry (sp_table_to_bytes)
 private:
  VarsAssignment() {}
};
// R1CSError::InvalidScalar (lib.rs:75-79) with what the check found: "InvalidScalar: entry <first> (<count> of <n> entries are not canonical)"
// From Instance::from_entries: "InvalidScalar: matrix <A|B|C> entry <first> (...)", matrix = 0, 1, 2 (-1 for an assignment); the report of
// that matrix is kept whole: report[0..1] = bad indices (count, lowest), report[2..3] = bad scalars among the entries with a good index.
struct InvalidScalar : Error {
  uint64_t first, count;
  int matrix = -1;
  uint64_t report[4] = {0, UINT64_MAX, 0, UINT64_MAX};
  InvalidScalar(uint64_t first, uint64_t count, size_t n);
  InvalidScalar(int matrix, const uint64_t report[4], size_t n);
};
// R1CSError::InvalidIndex (lib.rs:164-172) from Instance::from_entries: "InvalidIndex: matrix <A|B|C> entry <first> (<count> of <n> entries
// name a row or a column outside the instance)"
struct InvalidIndex : Error {
  uint64_t first, count;
  int matrix;
  uint64_t report[4];
  InvalidIndex(int matrix, const uint64_t report[4], size_t n);
};
// Assignment::new for inputs and other short vectors, on the calling thread: the same check, the same exception. scalars_to_bytes is
// Scalar::to_bytes of each.
FqVec scalars_from_bytes(const uint8_t* bytes, size_t n);
// Scalar::from_bytes (ristretto255.rs:390-416) accepts 32 little-endian bytes, read as four limbs, only when their value is below q: the
// host side's one statement of that test, from the top limb down
inline bool limbs_below_q(const uint64_t l[4]) {
  static const uint64_t Q[4] = {SP_Q0, SP_Q1, SP_Q2, SP_Q3};
  for (int w = 3; w >= 0; w--)
    if (l[w] != Q[w]) return l[w] < Q[w];
  return false;
}
std::vector<uint8_t> scalars_to_bytes(const Fq* s, size_t n);
// TEST/BENCH ONLY: from_bytes_wide(SHAKE256(domain || LE64(seed))[0..64]), the documented seed -> scalar map behind the
// reproducible RandomTape seeds of tests/ and bench.py. 64 bits of entropy: never a production tape seed.
Fq seed_scalar(const char* domain, uint64_t seed);

// zlib stream of `data` as miniz's tdefl produces it at level 6 (deflate.cc). old_header: 0x78 0x01 (miniz, miniz_oxide 0.3) instead of 0x78 0x9C
std::vector<uint8_t> zlib_level6_miniz(const uint8_t* data, size_t n, bool old_header = false);
// the same compressor at another probe count (tdefl flags & 0xFFF: 16/32/128/256/512/768/1500 = miniz levels 4..10); tests pin each against miniz
std::vector<uint8_t> zlib_miniz_probes(const uint8_t* data, size_t n, unsigned probes, bool old_header = false);
// The match search of that compressor as one independent item per input position (the rule: csrc/tdefl_rules.hpp, find; over whole tables
// on the host: deflate.cc; on the device: csrc/deflate_match.hip). A table entry is dist | len << 16, (0, init) when nothing was found:
//   L[p]  low 16 bits of the greatest q < p whose 3-byte hash equals p's, 0 if none (p + 2 < n; 0 elsewhere)
//   A[p]  the search at p that starts from nothing (init = 2)
//   B[p]  the search at p that has to beat A[p - 1], where A[p - 1] leaves the parser's filter as a held match; 0 elsewhere
// deflate_matches_host is the CPU yardstick and the fallback; L == nullptr: computed inside.
void deflate_links_host(const uint8_t* data, size_t n, uint16_t* L);
void deflate_matches_host(const uint8_t* data, size_t n, unsigned probes, const uint16_t* L, uint32_t* A, uint32_t* B);
// tdefl's parser, block decisions, Huffman coding and bit output (all sequential, all on the host) over such tables, segment by segment:
// a table look-up, the walk of tdefl_rules.hpp and the coder's step for each token it emits. parse(D, first, count, L, A, B) takes the
// tables of positions [first, first + count) — segments in order, without gaps — and needs D[0, min(n, first + count + 258)) readable. A
// lookup that neither table answers (a lazy chain of three or more matches whose held length is not A[p - 1]'s) is searched on the spot
// and counted in `fallbacks`.
struct MatchParser {
  MatchParser(size_t n, unsigned probes, bool old_header);
  ~MatchParser();
  MatchParser(const MatchParser&) = delete;
  void parse(const uint8_t* D, size_t first, size_t count, const uint16_t* L, const uint32_t* A, const uint32_t* B);
  std::vector<uint8_t> finish();  // the zlib stream; the parser is spent
  uint64_t lookups = 0, fallbacks = 0;
 private:
  struct Impl;
  Impl* m;
};
// one call over whole tables: equals zlib_miniz_probes(data, n, probes, old_header) byte for byte
std::vector<uint8_t> zlib_from_matches(const uint8_t* data, size_t n, const uint16_t* L, const uint32_t* A, const uint32_t* B, unsigned probes,
                                       bool old_header, uint64_t* lookups = nullptr, uint64_t* fallbacks = nullptr);
// The parse of that compressor restated as walks between free states (the rule: csrc/tdefl_rules.hpp, walk; on the device: the parse
// kernels of csrc/deflate_match.hip): one 32-bit token per literal or match, in stream order, laid out as tdefl_rules.hpp says (TOK_CHECK:
// tdefl's block check runs after this token; TOK_HELD: a match is held when it runs; TOK_VALID: always set).
using tdefl::TOK_VALID;
using tdefl::TOK_CHECK;
using tdefl::TOK_HELD;
// what deflate_tokens_host counts: conditions on an input that the tests ask for, not measurements
enum TokCounter { TOKC_WALKS, TOKC_LOOKUPS, TOKC_FALLBACKS, TOKC_FREE_LONG, TOKC_LIT_AND_LONG, TOKC_SPAN_TILE, TOKC_SPAN_GROUP, TOKC_SEAM_HELD,
                  TOKC_TOKENS, TOKC_MAX_JUMP, TOKC_COUNT };
// The token list of D[0, n) over the host tables of deflate_matches_host; tokens holds up to n entries; returns their number. geom (may be
// nullptr) = tile, tiles a group, segment length of the device parse this models: they change no token, only what the counters report —
// walks, look-ups, look-ups neither table answered, matches of >= 128 taken from a free state, a literal and a match of >= 128 from one
// step, matches spanning a tile / a group boundary inside a segment, segments entered with a held match, tokens, the longest jump F(p) - p.
size_t deflate_tokens_host(const uint8_t* data, size_t n, unsigned probes, const size_t geom[3], uint32_t* tokens, uint64_t counters[TOKC_COUNT]);
// tdefl's record_literal / record_match, block decisions, Huffman coding and bit output over such a token list, piece by piece (so that it
// runs behind the device parse): code(D, bytes_end, tokens, ntok) takes the next ntok tokens; D[0, bytes_end) has arrived (Adler-32, stored
// blocks) and covers every byte the tokens so far stand for.
struct TokenCoder {
  TokenCoder(size_t n, unsigned probes, bool old_header);
  ~TokenCoder();
  TokenCoder(const TokenCoder&) = delete;
  void code(const uint8_t* D, size_t bytes_end, const uint32_t* tokens, size_t ntok);
  std::vector<uint8_t> finish();  // the zlib stream; the coder is spent
  uint64_t tokens_coded = 0, full_blocks = 0, ratio_blocks = 0, stored_blocks = 0, static_blocks = 0;  // blocks ended by the code-buffer rule / the 115/128 rule
 private:
  struct Impl;
  Impl* m;
};
// one call over a whole list, fed `piece` tokens at a time (0: all at once): equals zlib_miniz_probes(data, n, probes, old_header) byte for byte.
// blocks (may be nullptr) = blocks ended by the code-buffer rule, by the 115/128 rule, stored blocks, static blocks
std::vector<uint8_t> zlib_from_tokens(const uint8_t* data, size_t n, const uint32_t* tokens, size_t ntok, unsigned probes, bool old_header,
                                      size_t piece = 0, uint64_t blocks[4] = nullptr);
// The coder split as the device runs it (csrc/deflate_emit.hip; the rules: csrc/tdefl_rules.hpp). A block record is BLOCK_REC 64-bit words —
// the index of the block's first token in the whole list, its tokens, its input bytes (total_lz_bytes), the rule that closed it
// (tdefl::BlockRule: 1 code buffer, 2 ratio, 3 finish), and the two numbers of flush_block's stored test, lookahead_pos - lz_dict_pos and
// dict_size after the block's last token (0, 0 for an empty block) — with BLOCK_HIST 16-bit counters beside it: 288 of the literal/length
// alphabet (the end-of-block symbol not counted), then 32 of the distances.
constexpr size_t BLOCK_REC = 6, BLOCK_HIST = 320, BLOCK_HDR_BYTES = 320;
// what deflate_blocks_host counts: conditions on an input and a segment length that the tests ask for
enum BlockCounter { BLKC_FULL, BLKC_RATIO, BLKC_EMPTY_FINAL, BLKC_SEAM_OPEN, BLKC_MAX_SPAN, BLKC_SEAM_AT_BOUNDARY, BLKC_MAX_TOKENS, BLKC_COUNT };
// The block records of a token list of n input bytes, found as the device finds them: segment by segment (tokens that start below a
// multiple of `segment`; 0: one segment), over the open block's carried tokens followed by the segment's, from inclusive sums of the token
// costs, by a chain of first-hit searches. records / hist hold `cap` blocks; returns their number (the last one is the finish block, which
// may be empty). counters (may be nullptr): blocks closed by the code-buffer rule, by the ratio rule, empty final blocks, seams an open
// block was carried over, the most segments one block touched, blocks whose last token was a segment's last, the most tokens of a block.
// Throws Error for a block of more than 58249 tokens.
size_t deflate_blocks_host(const uint32_t* tokens, size_t ntok, size_t n, size_t segment, uint64_t* records, uint16_t* hist, size_t cap,
                           uint64_t counters[BLKC_COUNT]);
enum BlockKind : uint32_t { BLOCK_DYNAMIC = 0, BLOCK_STATIC = 1, BLOCK_STORED = 2 };
// What the host decides about one block, from its record and histogram alone: where its bits go and what they are made of.
struct BlockPlan {
  uint64_t bit_off = 0;   // of the block's first bit (the final-block flag) in the stream
  uint64_t tok_off = 0;   // of its first token's bits; a stored block: of its first data byte (a multiple of 8)
  uint64_t eob_off = 0;   // of its end-of-block symbol (coded blocks)
  uint64_t end_off = 0;   // one past its last bit
  uint64_t src = 0, total = 0;  // the input bytes it stands for: D[src, src + total)
  uint32_t kind = 0, hdr_bits = 0;
  uint32_t table[BLOCK_HIST];   // code | size << 16 (tdefl::tok_bits); zeros for a stored block
  uint8_t hdr[BLOCK_HDR_BYTES]; // the bits from bit_off up to tok_off, first bit lowest: flag, type, and the dynamic header or LEN / NLEN
};
// Blocks in stream order: the unchanged optimize_table / start_dynamic_block / start_static_block for the tables and the header, the coded
// length from the histogram, flush_block's stored-or-coded test with the bit position carried from block to block, the offsets.
struct BlockPlanner {
  BlockPlanner(unsigned probes, bool old_header);
  ~BlockPlanner();
  BlockPlanner(const BlockPlanner&) = delete;
  void plan(const uint64_t* record, const uint16_t* hist, BlockPlan& p);
  size_t stream_bytes() const { return (size_t)((bitpos + 7) / 8) + 4; }  // after the finish block: the stream with its Adler-32 trailer
  void finish(std::vector<uint8_t>& z, uint32_t adler) const;            // z: the blocks' bits; sized, the zlib header and the trailer put in
  uint8_t head[2];
  uint64_t bitpos = 16, src = 0;
  uint64_t blocks = 0, stored_blocks = 0, static_blocks = 0, stored_after_midbyte = 0;

 private:
  struct Impl;
  Impl* m;
};
// the stream from block records: equals zlib_miniz_probes(data, n, probes, old_header) byte for byte. stats (may be nullptr; 3) = stored
// blocks, static blocks, stored blocks that follow a block ending within a byte
std::vector<uint8_t> zlib_from_blocks(const uint64_t* records, const uint16_t* hist, size_t nblocks, const uint32_t* tokens, const uint8_t* data, size_t n,
                                      unsigned probes, bool old_header, uint64_t stats[3]);
// zlib stream of n bytes at `data` (host memory) or `dev_data` (memory of the context's device), the matches searched on the device.
// parse: 0 = MatchParser over the downloaded tables, 1 = the parse on the device too and TokenCoder behind it, 2 = the coder's block
// boundaries, histograms and bit emission on the device as well and BlockPlanner behind it, -1 = as digest.device says (2: the device
// parse, 3: the device coder); tile, group: positions a tile and tiles a group of the device parse, chunk: tokens a workgroup of the
// emission (0: the library's defaults)
std::vector<uint8_t> zlib_device(sp_ctx* c, const uint8_t* data, const uint8_t* dev_data, size_t n, unsigned probes, bool old_header, DeflateStats* st,
                                 int parse = -1, size_t tile = 0, size_t group = 0, size_t chunk = 0);
// per-entry-point wall time of the option host.callstats (prover.cc), for driver files that cannot use its macro
void callstats_add(const char* entry, double seconds);

// ---- proof structs: field order == bincode order (same as the reference's serde derives) ----
struct PolyCommitment { std::vector<CP> C; };                                   // dense_mlpoly.rs:38-41
struct KnowledgeProof { CP alpha; Fq z1, z2; };                                 // nizk/mod.rs:15-20
struct EqualityProof { CP alpha; Fq z; };                                       // :77-81
struct ProductProof { CP alpha, beta, delta; Fq z[5]; };                        // :146-152
struct DotProductProof { CP delta, beta; FqVec z; Fq z_delta, z_beta; };        // :292-299
struct BulletReductionProof { std::vector<CP> L_vec, R_vec; };                  // bullet.rs:15-19
struct DotProductProofLog { BulletReductionProof bullet; CP delta, beta; Fq z1, z2; };  // nizk/mod.rs:421-428
struct PolyEvalProof { DotProductProofLog proof; };                             // dense_mlpoly.rs:303-306
struct ZKSumcheckInstanceProof { std::vector<CP> comm_polys, comm_evals; std::vector<DotProductProof> proofs; };  // sumcheck.rs:64-69
struct SumcheckInstanceProof { std::vector<FqVec> compressed_polys; };          // sumcheck.rs:17-20
struct R1CSProof {                                                              // r1csproof.rs:21-37
  PolyCommitment comm_vars;
  ZKSumcheckInstanceProof sc_proof_phase1;
  CP claims_phase2[4];
  KnowledgeProof pok_claims_phase2;
  ProductProof proof_prod;
  EqualityProof proof_eq_sc_phase1;
  ZKSumcheckInstanceProof sc_proof_phase2;
  CP comm_vars_at_ry;
  PolyEvalProof proof_eval_vars_at_ry;
  EqualityProof proof_eq_sc_phase2;
};
struct LayerProofBatched { SumcheckInstanceProof proof; FqVec claims_prod_left, claims_prod_right; };  // product_tree.rs:133-139
struct ProductCircuitEvalProofBatched { std::vector<LayerProofBatched> proof; FqVec claims_dotp[3]; };  // :162-166
struct ProductLayerProof {                                                      // sparse_mlpoly.rs:1021-1028
  Fq row_init; FqVec row_read, row_write; Fq row_audit;
  Fq col_init; FqVec col_read, col_write; Fq col_audit;
  FqVec eval_val[2];
  ProductCircuitEvalProofBatched proof_mem, proof_ops;
};
struct HashLayerProof {                                                         // :680-689
  FqVec row_addr, row_read_ts; Fq row_audit_ts;
  FqVec col_addr, col_read_ts; Fq col_audit_ts;
  FqVec eval_val;
  FqVec eval_derefs[2];
  PolyEvalProof proof_ops, proof_mem, proof_derefs;
};
struct SparseMatPolyEvalProof {                                                 // :1418-1422, :1307-1311
  PolyCommitment comm_derefs;
  ProductLayerProof proof_prod_layer;
  HashLayerProof proof_hash_layer;
};

// ---- SPARK dense representation on the device (sparse_mlpoly.rs:213-276) ----
struct DevIndex {  // Vec<usize> resident on the device
  sp_ctx* c = nullptr;
  sp_index* h = nullptr;
  DevIndex() {}
  DevIndex(sp_ctx* c_, sp_index* h_) : c(c_), h(h_) {}
  DevIndex(DevIndex&& o) noexcept : c(o.c), h(o.h) { o.h = nullptr; }
  DevIndex& operator=(DevIndex&& o) noexcept;
  DevIndex(const DevIndex&) = delete;
  ~DevIndex();
};
struct AddrTimestamps {
  std::vector<DevIndex> ops_addr_usize;
  std::vector<DevTable> ops_addr, read_ts;
  DevTable audit_ts;
};
struct MultiSparseMatPolynomialAsDense {
  size_t batch_size = 0, num_ops = 0, num_mem_cells = 0;
  std::vector<DevTable> val;
  AddrTimestamps row, col;
  DevTable comb_ops, comb_mem;
};
struct SparseMatPolyCommitment {  // :339-346
  size_t batch_size, num_ops, num_mem_cells;
  PolyCommitment comm_comb_ops, comm_comb_mem;
};
struct ComputationCommitment {  // lib.rs:44-48 -> r1cs.rs:50-56
  size_t num_cons, num_vars, num_inputs;
  SparseMatPolyCommitment comm;
  std::vector<uint8_t> serialize() const;  // bincode (r1cs.rs:50-56, sparse_mlpoly.rs:320-327, dense_mlpoly.rs:42-45)
  // the bytes serialize() writes, UNTRUSTED, into *out (verifier.cc): what a verifier holds of a circuit — it never has the decommitment. False
  // for truncated input, trailing bytes, a length that does not fit the bytes that remain, batch_size != 3, a share vector that is empty, not a
  // power of two or longer than 65536, or one whose size is not what encode gives for num_ops / num_mem_cells. Never throws.
  static bool deserialize(const uint8_t* bytes, size_t len, ComputationCommitment* out);
};
// The two share vectors of a ComputationCommitment as resident point sets of the device (sp_points: decoded once, window tables in HBM), for
// the verifier of many proofs over one circuit (spz_commitment_load makes them). SNARK::verify wants both: there is one path.
struct ResidentCommitment {
  const sp_points *ops = nullptr, *mem = nullptr;  // comm.comm_comb_ops.C, comm.comm_comb_mem.C
};
struct ComputationDecommitment {  // lib.rs:50-54 -> r1cs.rs:67-70
  MultiSparseMatPolynomialAsDense dense;
  // bincode of the serde-derived struct (sparse_mlpoly.rs:274-282, 212-218; dense_mlpoly.rs:17-22): every DensePolynomial is
  // {num_vars, len, Vec<Scalar>}; the tables are downloaded from the device (1.3 GB at 2^20: an interchange format, not a hot path)
  std::vector<uint8_t> serialize() const;
};

// The two halves of SNARK::encode (lib.rs:325-336), defined in the prover's sources (spark.inc, prover.cc) and shared with
// SNARK::encode_commitment (verifier.cc): the dense representation of the instance's matrices built on the device
// (MultiSparseMatPolynomialAsDense, sparse_mlpoly.rs:367-427 — no generators involved), and DensePolynomial::commit over the fixed-base tables
// of the prover's generators (dense_mlpoly.rs:179-204).
void encode_dense(Ctx& ctx, const Instance& inst, MultiSparseMatPolynomialAsDense* dense);
PolyCommitment poly_commit(sp_ctx* c, const DevTable& Z, size_t num_vars, const PolyCommitmentGens& gens, const FqVec* blinds);

struct ProveTimes {  // span names follow src/timer.rs call sites
  double polycommit = 0, sc_phase_one = 0, sc_phase_two = 0, polyeval = 0, r1cs_sat = 0, eval_sparse_polys = 0, commit_nondet_witness = 0,
         build_layered_network = 0, evalproof_layered_network = 0, total = 0;
};

struct SNARK {  // lib.rs:311-467
  R1CSProof r1cs_sat_proof;
  Fq inst_evals[3];
  SparseMatPolyEvalProof r1cs_eval_proof;
  // SNARK::encode (lib.rs:325-336)
  static void encode(Ctx& ctx, const Instance& inst, const SNARKGens& gens, ComputationCommitment* comm, ComputationDecommitment* decomm);
  // The commitment half of encode alone, under EITHER kind of generators (verifier.cc): the dense representation is built, comb_ops and comb_mem
  // are committed and the tables are let go — no decommitment is kept. What a process that only verifies runs to obtain the commitment of
  // the circuit it verifies against, instead of trusting bytes handed to it: under verifier-only generators the row commitments are flat sums
  // over gens_ops' / gens_mem's range of stream_eval's resident point set, under the prover's they go through the window tables as in
  // encode. The same bytes either way, and encode's.
  static ComputationCommitment encode_commitment(Ctx& ctx, const Instance& inst, const SNARKGens& gens);
  // SNARK::prove (lib.rs:339-420). tape_seed == nullptr: the RandomTape is seeded from OS entropy like RandomTape::new
  // (random.rs:13-15) — the production setting. A non-null seed is the `new_with_seed` test hook: it determines every blind,
  // so it must be secret, >= 256 bits of entropy and single-use, or the proof is no longer zero-knowledge.
  static SNARK prove(Ctx& ctx, const Instance& inst, const ComputationCommitment& comm, const ComputationDecommitment& decomm,
                     const FqVec& vars, const FqVec& inputs, const SNARKGens& gens, Transcript& transcript, const Fq* tape_seed,
                     ProveTimes* times = nullptr) {
    return prove(ctx, inst, comm, decomm, vars.data(), vars.size(), inputs, gens, transcript, tape_seed, times);
  }
  // same, reading the assignment in place (a Rust `&[Scalar]` / a caller-owned buffer): no host-side copy
  static SNARK prove(Ctx& ctx, const Instance& inst, const ComputationCommitment& comm, const ComputationDecommitment& decomm,
                     const Fq* vars, size_t num_vars_given, const FqVec& inputs, const SNARKGens& gens, Transcript& transcript,
                     const Fq* tape_seed, ProveTimes* times = nullptr, const sp_table* vars_resident = nullptr);
  // same, from an assignment already in HBM
  static SNARK prove(Ctx& ctx, const Instance& inst, const ComputationCommitment& comm, const ComputationDecommitment& decomm,
                     const VarsAssignment& vars, const FqVec& inputs, const SNARKGens& gens, Transcript& transcript, const Fq* tape_seed,
                     ProveTimes* times = nullptr) {
    return prove(ctx, inst, comm, decomm, nullptr, vars.n, inputs, gens, transcript, tape_seed, times, vars.tab.h);
  }
  std::vector<uint8_t> serialize() const;  // bincode 1.3 default encoding
  // bincode of an UNTRUSTED proof into *out (verifier.cc), under the rules of NIZK::deserialize: every Vec length — the nested Vec<Vec<Scalar>> of
  // compressed_polys and the Vec<LayerProofBatched> included — is checked against the bytes that remain before anything is allocated. Never throws.
  static bool deserialize(const uint8_t* bytes, size_t len, SNARK* out);
  // SNARK::verify (lib.rs:423-466) against a computation commitment: 1 accept, 0 reject. R1CSProof::verify takes the proof's inst_evals, the
  // sparse-polynomial evaluation proof binds them to the commitment; the four C_LZ multi-scalar multiplications run on the device (placement:
  // verifier.cc). Throws Error("InvalidNumberOfInputs") for a wrong number of inputs (lib.rs:437), Error for a device failure; a proof that is
  // merely wrong, has a vector of the wrong length, or carries undecodable points, is a 0.
  int verify(Ctx& ctx, const ComputationCommitment& comm, const FqVec& inputs, Transcript& transcript, const SNARKGens& gens,
             const ResidentCommitment& resident) const;
  // K UNTRUSTED proofs (bytes, length) of one circuit, each verified by verify() itself under a transcript of its own made from
  // `transcript_label`, one host thread a proof, in lock step: the threads meet at the three blocking device calls of a verification
  // (batch_gate.hpp) and the requests of one shape go out as ONE call (sp_msm_var_many, sp_msm_points_many, sp_commit_rows with rows = K) — 8
  // round trips for a batch of up to 64 proofs instead of 8 each. No combined equation: every proof gets the verdict verify() gives it, 1 accept,
  // 0 reject, -1 malformed bytes (these never start a thread); a proof that is rejected leaves the lock step without holding the others up.
  // Lists longer than 64 are cut into batches of 64. inputs[k] belongs to proofs[k]. Throws Error("InvalidNumberOfInputs") before anything
  // runs when one of them has another size than the commitment's; Error for a device failure (then no verdict is given at all).
  static std::vector<int> verify_many(Ctx& ctx, const ComputationCommitment& comm, const std::vector<std::pair<const uint8_t*, size_t>>& proofs,
                                      const std::vector<const FqVec*>& inputs, const char* transcript_label, const SNARKGens& gens,
                                      const ResidentCommitment& resident);
};
struct NIZK {  // lib.rs:488-587
  R1CSProof r1cs_sat_proof;
  FqVec rx, ry;
  static NIZK prove(Ctx& ctx, const Instance& inst, const FqVec& vars, const FqVec& inputs, const NIZKGens& gens, Transcript& transcript,
                    const Fq* tape_seed, ProveTimes* times = nullptr) {
    return prove(ctx, inst, vars.data(), vars.size(), inputs, gens, transcript, tape_seed, times);
  }
  static NIZK prove(Ctx& ctx, const Instance& inst, const Fq* vars, size_t num_vars_given, const FqVec& inputs, const NIZKGens& gens,
                    Transcript& transcript, const Fq* tape_seed, ProveTimes* times = nullptr, const sp_table* vars_resident = nullptr);
  static NIZK prove(Ctx& ctx, const Instance& inst, const VarsAssignment& vars, const FqVec& inputs, const NIZKGens& gens, Transcript& transcript,
                    const Fq* tape_seed, ProveTimes* times = nullptr) {
    return prove(ctx, inst, nullptr, vars.n, inputs, gens, transcript, tape_seed, times, vars.tab.h);
  }
  std::vector<uint8_t> serialize() const;
  // bincode of an UNTRUSTED proof into *out (verifier.cc): false for anything that is not exactly one NIZK — a length that does not fit the
  // bytes that remain (checked before allocating), a scalar whose limbs are >= q, truncated input, trailing bytes. Never throws.
  static bool deserialize(const uint8_t* bytes, size_t len, NIZK* out);
  // NIZK::verify (lib.rs:549-587): 1 accept, 0 reject. The instance's digest is absorbed as NIZK::prove absorbs it; R1CSInstance::evaluate and the
  // table-sized group operations run on the device (placement: verifier.cc). Throws Error("InvalidNumberOfInputs") for a wrong number of
  // inputs (lib.rs:569), Error for a device failure; a proof that is merely wrong, or carries undecodable points, is a 0.
  int verify(Ctx& ctx, const Instance& inst, const FqVec& inputs, Transcript& transcript, const NIZKGens& gens) const;
  // K UNTRUSTED proofs (bytes, length) of one instance, under the conventions of SNARK::verify_many: verify() itself per proof, one host thread
  // and one transcript each, in lock step through a gate. C_LZ and G_hat go out as one call a batch; R1CSInstance::evaluate at the K proofs'
  // own points is ONE sp_sparse_evaluate_many_begin that reads every matrix entry once and builds no full chi table. The job belongs to the
  // batch: a proof that is rejected early neither waits for it nor frees it. Verdicts 1 accept, 0 reject, -1 malformed bytes (these never start
  // a thread). Lists longer than 64 are cut into batches of 64; the instance's digest is computed once per call. Throws
  // Error("InvalidNumberOfInputs") before anything runs; Error for a device failure (then no verdict is given at all).
  static std::vector<int> verify_many(Ctx& ctx, const Instance& inst, const std::vector<std::pair<const uint8_t*, size_t>>& proofs,
                                      const std::vector<const FqVec*>& inputs, const char* transcript_label, const NIZKGens& gens);
};

std::vector<uint8_t> serialize_r1cs_proof(const R1CSProof& p);

// Where the few-term commitments of the Sigma protocols run: on the proving thread's core through the library's host-side
// engine (sp_host_commit_small / sp_host_zk_ahead_*, csrc/host_commit.hip — the default) or on the GPU (sp_msm_indexed;
// option commit.small_device = 1). Byte-identical proofs either way.
inline bool small_msm_on_host(const sp_ctx* c) { return ctx_opt(c, "commit.small_device") == 0; }

}  // namespace spz
