// spartan_amd host driver: C entry points over libspartan.hpp for ctypes (tests/, bench.py). Exceptions are
// turned into NULL / error strings here; nothing throws across the boundary.
#include <cstring>
#include <memory>
#include <string>

#include "libspartan.hpp"
#include "fq_inv.hpp"

using namespace spz;

namespace {
thread_local std::string g_err;
struct EncH { ComputationCommitment comm; ComputationDecommitment decomm; };
struct ProofH { std::vector<uint8_t> bytes; };
struct CommH {  // what spz_commitment_load hands out: the commitment and its two share vectors as resident point sets
  ComputationCommitment comm;
  sp_points *ops = nullptr, *mem = nullptr;
  ~CommH() { sp_points_free(ops); sp_points_free(mem); }
};
FqVec limbs_vec(const uint64_t* p, size_t n) { FqVec v(n); if (n) memcpy(v[0].l, p, 32 * n); return v; }
void fill_times(const ProveTimes& t, double* o) {
  if (!o) return;
  o[0] = t.polycommit; o[1] = t.sc_phase_one; o[2] = t.sc_phase_two; o[3] = t.polyeval; o[4] = t.r1cs_sat; o[5] = t.eval_sparse_polys;
  o[6] = t.commit_nondet_witness; o[7] = t.build_layered_network; o[8] = t.evalproof_layered_network; o[9] = t.total;
}
// A generator handle where the PROVER's generators are needed (encode, every prove, the window-table accessors): a verifier-only handle
// (spz_*_verifier_gens_new) is refused here, before any device call — it has no sp_gens, and a null one must never reach a kernel.
template <typename G>
G& prover_gens(void* gens, const char* what) {
  if (!gens) throw Error(std::string(what) + ": bad arguments");
  G& g = *(G*)gens;
  if (g.is_verifier_only()) throw Error(std::string(what) + ": verifier-only generators (they verify; they hold no fixed-base window tables)");
  return g;
}
template <typename F>
auto guard(F f) -> decltype(f()) {
  try {
    g_err.clear();
    return f();
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
// guard for the parsers of canonical scalar bytes: the report of the check goes out on success ((0, UINT64_MAX)) and on InvalidScalar alike
template <typename F>
auto scalar_guard(uint64_t* report, F f) -> decltype(f()) {
  try {
    g_err.clear();
    auto r = f();
    if (report) { report[0] = 0; report[1] = UINT64_MAX; }
    return r;
  } catch (const InvalidScalar& e) {
    if (report) { report[0] = e.count; report[1] = e.first; }
    g_err = e.what();
  } catch (const std::exception& e) {
    g_err = e.what();
  }
  return decltype(f())();
}
// guard of the instance constructors that parse an entry list on the device: status, failing matrix and that matrix's report go out either way
template <typename F>
void* entries_guard(int32_t* status, int* matrix, uint64_t* report, F f) {
  int32_t st = SP_EINVAL;
  int mat = -1;
  uint64_t rep[4] = {0, UINT64_MAX, 0, UINT64_MAX};
  void* h = nullptr;
  try {
    g_err.clear();
    h = f();
    st = SP_OK;
  } catch (const InvalidIndex& e) {
    st = SP_EINDEX; mat = e.matrix; memcpy(rep, e.report, sizeof rep);
    g_err = e.what();
  } catch (const InvalidScalar& e) {
    st = SP_ESCALAR; mat = e.matrix; memcpy(rep, e.report, sizeof rep);
    g_err = e.what();
  } catch (const std::exception& e) {
    g_err = e.what();
  }
  if (status) *status = st;
  if (matrix) *matrix = mat;
  if (report) memcpy(report, rep, sizeof rep);
  return h;
}
}  // namespace

extern "C" {
const char* spz_last_error() { return g_err.c_str(); }
void* spz_ctx_new(int device) { return guard([&]() -> void* { return new Ctx(device); }); }
void spz_ctx_free(void* c) { delete (Ctx*)c; }
sp_ctx* spz_ctx_raw(void* c) { return ((Ctx*)c)->h; }
// row-sharded commitments across `world` lock-step ranks (libspartan.hpp: set_commit_shard); 0 = ok
int spz_ctx_set_commit_shard(void* c, int rank, int world, CommitGatherFn gather, void* user) {
  try {
    set_commit_shard(*(Ctx*)c, rank, world, gather, user);
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// RCCL inside the library (shard.cc): rank 0 draws the id, the caller distributes it, every rank joins; 0 = ok
int spz_rccl_unique_id(uint8_t out[128]) {
  try { rccl_unique_id(out); return 0; } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int spz_ctx_set_commit_shard_rccl(void* c, int rank, int world, const uint8_t unique_id[128]) {
  try { set_commit_shard_rccl(*(Ctx*)c, rank, world, unique_id); return 0; } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// W shards on one GPU, in-process gather (the partitioning logic without a second GPU); nshards <= 1 clears it
int spz_ctx_set_commit_shard_virtual(void* c, int nshards) {
  try { set_commit_shard_virtual(*(Ctx*)c, nshards); return 0; } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
double spz_rccl_allgather_probe(void* c, size_t bytes, int iters) {
  try { return rccl_allgather_probe(((Ctx*)c)->h, bytes, iters); } catch (const std::exception& e) { g_err = e.what(); return -2.0; }
}
void spz_ctx_shard_stats(void* c, int reset, uint64_t out[2]) {
  ShardStats s = commit_shard_stats(*(Ctx*)c, reset != 0);
  out[0] = s.gathers; out[1] = s.bytes;
}

// Instance::new (lib.rs:121-128): entries of A, B, C back to back as (row, col, [u8;32] canonical little-endian value).
// Errors mirror R1CSError: "InvalidIndex", "InvalidScalar" (spz_last_error()).
void* spz_instance_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* rows,
                       const uint64_t* cols, const uint8_t* vals) {
  return guard([&]() -> void* {
    std::vector<SparseEntry> m[3];
    // lib.rs:164-186: an entry is checked for InvalidIndex first, then its scalar for InvalidScalar
    size_t off = 0;
    for (int k = 0; k < 3; k++)
      for (size_t i = 0; i < nnz[k]; i++, off++) {
        SparseEntry e;
        e.row = rows[off]; e.col = cols[off];
        if (e.row >= num_cons || e.col >= num_vars + 1 + num_inputs) throw Error("InvalidIndex");
        sp::Fq raw;
        memcpy(raw.l, vals + 32 * off, 32);
        // Scalar::from_bytes (ristretto255.rs:390-416): reject encodings >= q
        static const uint64_t Q[4] = {SP_Q0, SP_Q1, SP_Q2, SP_Q3};
        bool lt = false;
        for (int w = 3; w >= 0; w--) {
          if (raw.l[w] != Q[w]) { lt = raw.l[w] < Q[w]; break; }
        }
        if (!lt) throw Error("InvalidScalar");
        e.val = sp::fq_to_mont(raw);
        m[k].push_back(e);
      }
    return new Instance(*(Ctx*)ctx, num_cons, num_vars, num_inputs, m[0], m[1], m[2]);
  });
}
// Instance::new on the device (Instance::from_entries): the same arguments as spz_instance_new, and the same two errors, with what the check
// found. NULL on failure; *status (may be NULL) = SP_OK, SP_EINDEX ("InvalidIndex: ..."), SP_ESCALAR ("InvalidScalar: ...") or SP_EINVAL for
// anything else; *matrix (may be NULL) = 0, 1, 2 for the matrix that failed, -1 otherwise; report (may be NULL, 4 words) = that matrix's report as
// sp_sparse_from_entries gives it, (0, UINT64_MAX, 0, UINT64_MAX) on success.
void* spz_instance_from_entries(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* rows,
                                const uint64_t* cols, const uint8_t* vals, int32_t* status, int* matrix, uint64_t report[4]) {
  return entries_guard(status, matrix, report, [&]() -> void* {
    if (!ctx || !nnz) throw Error("spz_instance_from_entries: bad arguments");
    return Instance::from_entries(*(Ctx*)ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals).release();
  });
}
// The same from device memory: rows[k], cols[k], vals[k] are the three lists of matrix k in the memory of the context's device, written and
// complete before the call.
void* spz_instance_from_device_entries(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* const rows[3],
                                       const uint64_t* const cols[3], const uint8_t* const vals[3], int32_t* status, int* matrix, uint64_t report[4]) {
  return entries_guard(status, matrix, report, [&]() -> void* {
    if (!ctx || !nnz || !rows || !cols || !vals) throw Error("spz_instance_from_device_entries: bad arguments");
    return Instance::from_device_entries(*(Ctx*)ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals).release();
  });
}
// Instance::produce_synthetic_r1cs with a seed; vars (num_vars) and inputs (num_inputs) are written out
void* spz_instance_synthetic(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, uint64_t seed, uint64_t* vars_out, uint64_t* inputs_out) {
  return guard([&]() -> void* {
    FqVec v, in;
    std::unique_ptr<Instance> p = Instance::produce_synthetic_r1cs(*(Ctx*)ctx, num_cons, num_vars, num_inputs, seed, &v, &in);
    if (vars_out) memcpy(vars_out, v[0].l, 32 * v.size());
    if (inputs_out && !in.empty()) memcpy(inputs_out, in[0].l, 32 * in.size());
    return p.release();
  });
}
// UniPoly::from_evals / compress / evaluate (unipoly.rs) on n = 3 or 4 evaluations; scalars as Montgomery limbs. Test hook.
// host arithmetic of the batched cubic sum-check (spark.inc): the cubic in the next challenge, and the last rounds on short tables
void spz_cubic_coeffs_probe(const uint64_t S[48], const uint64_t r[4], uint64_t ev[12]) {
  Fq s[12], rr, e[3];
  memcpy(s, S, sizeof s); memcpy(rr.l, r, 32);
  cubic_coeffs_probe(s, rr, e);
  memcpy(ev, e, sizeof e);
}
// tab: [ni][3][m] in, bound in place; evs: 3 per round (log2 m rounds); returns the number of rounds
int spz_cubic_tail_probe(uint64_t* tab, size_t ni, size_t m, const uint64_t* coeffs, const uint64_t* challenges, uint64_t* evs) {
  size_t rounds = 0;
  for (size_t x = m; x > 1; x /= 2) rounds++;
  FqVec t = limbs_vec(tab, ni * 3 * m), cf = limbs_vec(coeffs, ni), ch = limbs_vec(challenges, rounds), e;
  cubic_tail_probe(t, ni, m, cf, ch, &e);
  memcpy(tab, t.data(), 32 * t.size());
  memcpy(evs, e.data(), 32 * e.size());
  return (int)rounds;
}
int spz_eq_factor_probe(const uint64_t* rho, size_t nvars, size_t np, size_t ni, const uint64_t* coeffs, size_t nrounds, const uint64_t* claims,
                        const uint64_t* ev4, const uint64_t* challenges, uint64_t* evc_out, uint64_t* K_out) {
  auto vec = [](const uint64_t* p, size_t n) { FqVec v(n); memcpy(v.data(), p, 32 * n); return v; };
  FqVec evc, K;
  if (!eq_factor_probe(vec(rho, nvars), np, ni, vec(coeffs, ni), vec(claims, nrounds), vec(ev4, 4 * ni * nrounds), vec(challenges, nrounds), &evc, &K)) return 0;
  memcpy(evc_out, evc.data(), 32 * evc.size());
  memcpy(K_out, K.data(), 32 * K.size());
  return 1;
}
int spz_unipoly_probe(const uint64_t* evals, size_t n, const uint64_t r[4], uint64_t* coeffs, uint64_t* compressed, uint64_t eval_at_r[4]) {
  try {
    FqVec e(n), c, cc;
    memcpy(e.data(), evals, 32 * n);
    Fq rr, ev;
    memcpy(rr.l, r, 32);
    unipoly_probe(e, rr, &c, &cc, &ev);
    memcpy(coeffs, c.data(), 32 * c.size());
    memcpy(compressed, cc.data(), 32 * cc.size());
    memcpy(eval_at_r, ev.l, 32);
    return 0;
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return -1;
  }
}
// test hook: the challenge inversion of the inner-product rounds (fq_inv.hpp), Montgomery limbs in and out
void spz_fq_invert_vartime(const uint64_t in[4], uint64_t out[4]) { Fq a; memcpy(a.l, in, 32); Fq r = fq_invert_vartime(a); memcpy(out, r.l, 32); }
void spz_seed_scalar(const char* domain, uint64_t seed, uint64_t out[4]) { Fq s = seed_scalar(domain, seed); memcpy(out, s.l, 32); }
void spz_instance_set_digest(void* inst, const uint8_t* d, size_t n) { ((Instance*)inst)->set_digest(d, n); }
// zlib header variant of the COMPUTED digest: 0 = 0x78 0x9C (miniz >= 2.2, miniz_oxide >= 0.4: FLEVEL from the level), 1 = 0x78 0x01 (older).
// An explicit parameter of the instance (not an environment switch); call before the digest is first used.
int spz_instance_set_digest_header(void* inst, int old_header) {  // 0 = ok, -1 = a digest with the other header has already been computed (or set)
  if (((Instance*)inst)->set_digest_header(old_header != 0)) return 0;
  g_err = "set_digest_header after the digest was first used";
  return -1;
}
// R1CSShape::get_digest (r1cs.rs:154-158): the zlib stream; and the bincode it compresses (for the round-trip tests)
size_t spz_instance_digest(void* inst, uint8_t* out, size_t cap) {
  const std::vector<uint8_t> d = ((Instance*)inst)->compute_digest();
  if (out && cap >= d.size()) memcpy(out, d.data(), d.size());
  return d.size();
}
size_t spz_instance_shape_bincode(void* inst, uint8_t* out, size_t cap) {
  std::vector<uint8_t> b = ((Instance*)inst)->shape_bincode();
  if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
  return b.size();
}
// the deflater alone (CPU tests): zlib_level6_miniz of arbitrary bytes
size_t spz_zlib_level6(const uint8_t* data, size_t n, int old_header, uint8_t* out, size_t cap) {
  std::vector<uint8_t> z = zlib_level6_miniz(data, n, old_header != 0);
  if (out && cap >= z.size()) memcpy(out, z.data(), z.size());
  return z.size();
}
// the same deflater at another tdefl probe count (miniz levels 4..10 = 16/32/128/256/512/768/1500): pinned per level against the real miniz
size_t spz_zlib_probes(const uint8_t* data, size_t n, unsigned probes, int old_header, uint8_t* out, size_t cap) {
  std::vector<uint8_t> z = zlib_miniz_probes(data, n, probes, old_header != 0);
  if (out && cap >= z.size()) memcpy(out, z.data(), z.size());
  return z.size();
}
void spz_instance_free(void* i) { delete (Instance*)i; }
void* spz_snark_gens_new(void* ctx, size_t nc, size_t nv, size_t ni, size_t nnz) {
  return guard([&]() -> void* { return new SNARKGens(*(Ctx*)ctx, nc, nv, ni, nnz); });
}
// the verifier's generators (libspartan.hpp: SNARKGens::verifier_only): the same handle type, taken by every spz_snark_verify* entry and by
// spz_snark_gens_stream; refused by spz_snark_encode, every spz_snark_prove* and the window-table accessors
void* spz_snark_verifier_gens_new(void* ctx, size_t nc, size_t nv, size_t ni, size_t nnz) {
  return guard([&]() -> void* { return new SNARKGens(SNARKGens::verifier_only(*(Ctx*)ctx, nc, nv, ni, nnz)); });
}
int spz_snark_gens_is_verifier_only(void* g) { return ((SNARKGens*)g)->is_verifier_only() ? 1 : 0; }
size_t spz_snark_gens_resident_bytes(void* g) { return ((SNARKGens*)g)->resident_bytes(); }  // HBM held by the tables of both streams, either kind
void spz_snark_gens_free(void* g) { delete (SNARKGens*)g; }
void* spz_nizk_gens_new(void* ctx, size_t nc, size_t nv, size_t ni) {
  return guard([&]() -> void* { return new NIZKGens(*(Ctx*)ctx, nc, nv, ni); });
}
void* spz_nizk_verifier_gens_new(void* ctx, size_t nc, size_t nv, size_t ni) {  // NIZKGens::verifier_only: for spz_nizk_verify*; refused by spz_nizk_prove*
  return guard([&]() -> void* { return new NIZKGens(NIZKGens::verifier_only(*(Ctx*)ctx, nc, nv, ni)); });
}
int spz_nizk_gens_is_verifier_only(void* g) { return ((NIZKGens*)g)->is_verifier_only() ? 1 : 0; }
size_t spz_nizk_gens_resident_bytes(void* g) { return ((NIZKGens*)g)->resident_bytes(); }
void spz_nizk_gens_free(void* g) { delete (NIZKGens*)g; }
// compressed points of the two generator streams (for parity checks against the oracle's MultiCommitGens)
size_t spz_snark_gens_stream(void* g, int which, uint8_t* out, size_t cap) {
  const std::vector<uint8_t>& v = which == 0 ? ((SNARKGens*)g)->stream_sat.compressed : ((SNARKGens*)g)->stream_eval.compressed;
  if (out && cap >= v.size()) memcpy(out, v.data(), v.size());
  return v.size();
}
// library options of the context (include/spartan_hip.h: sp_ctx_set_option); ctx == NULL: the process-wide defaults
int spz_ctx_set_option(void* ctx, const char* key, const char* value) { return sp_ctx_set_option(ctx ? ((Ctx*)ctx)->h : nullptr, key, value); }
// window width of the fixed-base tables of a generator stream (0: gens_r1cs_sat, 1: gens_r1cs_eval)
// (a verifier-only handle has no such tables: -1 / 0 with spz_last_error())
static const sp_gens* window_tables_of(void* g, int which, const char* what) {
  try {
    g_err.clear();
    SNARKGens& G = prover_gens<SNARKGens>(g, what);
    return which == 0 ? G.stream_sat.g : G.stream_eval.g;
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
int spz_snark_gens_window_bits(void* g, int which) { const sp_gens* t = window_tables_of(g, which, "spz_snark_gens_window_bits"); return t ? sp_gens_window_bits(t) : -1; }
int spz_snark_gens_windows(void* g, int which) { const sp_gens* t = window_tables_of(g, which, "spz_snark_gens_windows"); return t ? sp_gens_windows(t) : -1; }
size_t spz_snark_gens_table_bytes(void* g, int which) { const sp_gens* t = window_tables_of(g, which, "spz_snark_gens_table_bytes"); return t ? sp_gens_table_bytes(t) : 0; }
// bincode of SNARKGens / ComputationCommitment (wire formats)
size_t spz_snark_gens_bincode(void* g, uint8_t* out, size_t cap) {
  std::vector<uint8_t> b = ((SNARKGens*)g)->serialize();
  if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
  return b.size();
}
size_t spz_commitment_bincode(void* e, uint8_t* out, size_t cap);
void* spz_snark_encode(void* ctx, void* inst, void* gens) {
  return guard([&]() -> void* {
    SNARKGens* pg = &prover_gens<SNARKGens>(gens, "spz_snark_encode");
    EncH* e = new EncH;
    try {
      SNARK::encode(*(Ctx*)ctx, *(Instance*)inst, *pg, &e->comm, &e->decomm);
    } catch (...) {
      delete e;
      throw;
    }
    return e;
  });
}
void spz_encode_free(void* e) { delete (EncH*)e; }
size_t spz_commitment_bincode(void* e, uint8_t* out, size_t cap) {
  std::vector<uint8_t> b = ((EncH*)e)->comm.serialize();
  if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
  return b.size();
}
// bincode(ComputationDecommitment): returns the size; fills out when cap suffices
size_t spz_decommitment_bincode(void* e, uint8_t* out, size_t cap) {
  try {
    std::vector<uint8_t> b = ((EncH*)e)->decomm.serialize();
    if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
    return b.size();
  } catch (const std::exception& ex) {
    g_err = ex.what();
    return 0;
  }
}
size_t spz_encode_comm(void* ev, int which, uint8_t* out, size_t cap) {
  EncH* e = (EncH*)ev;
  const PolyCommitment& c = which == 0 ? e->comm.comm.comm_comb_ops : e->comm.comm.comm_comb_mem;
  if (out && cap >= 32 * c.C.size())
    for (size_t i = 0; i < c.C.size(); i++) memcpy(out + 32 * i, c.C[i].data(), 32);
  return c.C.size();
}
void* spz_snark_prove(void* ctx, void* inst, void* gens, void* enc, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                      const char* transcript_label, const uint64_t tape_seed[4], double* times10) {
  return guard([&]() -> void* {
    SNARKGens& G = prover_gens<SNARKGens>(gens, "spz_snark_prove");
    Transcript t(transcript_label);
    Fq seed;  // tape_seed == NULL: RandomTape::new, seeded from OS entropy (random.rs:13-15)
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    EncH* e = (EncH*)enc;
    SNARK p = SNARK::prove(*(Ctx*)ctx, *(Instance*)inst, e->comm, e->decomm, (const sp::Fq*)vars, nvars, limbs_vec(inputs, ninputs), G,
                           t, tape_seed ? &seed : nullptr, &tm);
    fill_times(tm, times10);
    ProofH* h = new ProofH;
    h->bytes = p.serialize();
    return h;
  });
}
// SNARK::prove / NIZK::prove on a CALLER-OWNED transcript (src/lib.rs:339-347, 501-509: `transcript: &mut Transcript`): the
// 203 bytes of the merlin transcript (STROBE state, pos, pos_begin, cur_flags) come in, the proof is produced on their
// continuation, and the state after the proof goes back so the caller's transcript can carry on — whatever it had absorbed
// before. `assignment` (a spz_vars_assignment_new handle) or `vars` (host scalars), one of them. This is the entry the Rust
// crate's SNARK::prove / NIZK::prove call under `--features gpu` (rust_shim/seams/lib.rs).
void* spz_snark_prove_t(void* ctx, void* inst, void* gens, void* enc, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs,
                        size_t ninputs, uint8_t transcript_state[203], const uint64_t tape_seed[4], double* times10) {
  return guard([&]() -> void* {
    SNARKGens& G = prover_gens<SNARKGens>(gens, "spz_snark_prove_t");
    if (!transcript_state || (!assignment && !vars)) throw Error("spz_snark_prove_t: bad arguments");
    Transcript t(Transcript::FromState(), transcript_state);
    Fq seed;
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    EncH* e = (EncH*)enc;
    SNARK p = assignment ? SNARK::prove(*(Ctx*)ctx, *(Instance*)inst, e->comm, e->decomm, *(VarsAssignment*)assignment, limbs_vec(inputs, ninputs),
                                        G, t, tape_seed ? &seed : nullptr, &tm)
                         : SNARK::prove(*(Ctx*)ctx, *(Instance*)inst, e->comm, e->decomm, (const sp::Fq*)vars, nvars, limbs_vec(inputs, ninputs),
                                        G, t, tape_seed ? &seed : nullptr, &tm);
    fill_times(tm, times10);
    ProofH* h = new ProofH;
    h->bytes = p.serialize();
    t.export_state(transcript_state);
    return h;
  });
}
void* spz_nizk_prove_t(void* ctx, void* inst, void* gens, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                       uint8_t transcript_state[203], const uint64_t tape_seed[4], double* times10) {
  return guard([&]() -> void* {
    NIZKGens& G = prover_gens<NIZKGens>(gens, "spz_nizk_prove_t");
    if (!transcript_state || (!assignment && !vars)) throw Error("spz_nizk_prove_t: bad arguments");
    Transcript t(Transcript::FromState(), transcript_state);
    Fq seed;
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    NIZK p = assignment ? NIZK::prove(*(Ctx*)ctx, *(Instance*)inst, *(VarsAssignment*)assignment, limbs_vec(inputs, ninputs), G, t,
                                      tape_seed ? &seed : nullptr, &tm)
                        : NIZK::prove(*(Ctx*)ctx, *(Instance*)inst, (const sp::Fq*)vars, nvars, limbs_vec(inputs, ninputs), G, t,
                                      tape_seed ? &seed : nullptr, &tm);
    fill_times(tm, times10);
    ProofH* h = new ProofH;
    h->bytes = p.serialize();
    t.export_state(transcript_state);
    return h;
  });
}
// VarsAssignment::new: the assignment uploaded once; spz_*_prove_resident prove from the device copy
void* spz_vars_assignment_new(void* ctx, const uint64_t* vars, size_t nvars) {
  return guard([&]() -> void* { return new VarsAssignment(*(Ctx*)ctx, (const sp::Fq*)vars, nvars); });
}
void spz_vars_assignment_free(void* a) { delete (VarsAssignment*)a; }
// Assignment::new (lib.rs:62-88) as the reference takes it: 32 * n canonical little-endian bytes, in host memory (_from_bytes) or in the memory of
// the context's device (_from_device_bytes: the caller has completed the writes), parsed on the device into an ordinary resident assignment.
// NULL with spz_last_error() beginning "InvalidScalar" when an entry is >= q. report (may be NULL), on success and on that failure alike:
// report[0] = entries >= q, report[1] = the lowest such index (UINT64_MAX when none).
void* spz_vars_assignment_from_bytes(void* ctx, const uint8_t* bytes, size_t n, uint64_t report[2]) {
  return scalar_guard(report, [&]() -> void* {
    if (!ctx) throw Error("spz_vars_assignment_from_bytes: bad arguments");
    return new VarsAssignment(VarsAssignment::from_bytes(*(Ctx*)ctx, bytes, n));
  });
}
void* spz_vars_assignment_from_device_bytes(void* ctx, const uint8_t* dev, size_t n, uint64_t report[2]) {
  return scalar_guard(report, [&]() -> void* {
    if (!ctx) throw Error("spz_vars_assignment_from_device_bytes: bad arguments");
    return new VarsAssignment(VarsAssignment::from_device_bytes(*(Ctx*)ctx, dev, n));
  });
}
size_t spz_vars_assignment_len(void* a) { return a ? ((VarsAssignment*)a)->n : 0; }
// Scalar::to_bytes of every entry: out receives 32 * spz_vars_assignment_len(a) bytes. 0 = ok, -1 = error (spz_last_error()).
int spz_vars_assignment_to_bytes(void* a, uint8_t* out) {
  try {
    g_err.clear();
    if (!a || !out) throw Error("spz_vars_assignment_to_bytes: bad arguments");
    const std::vector<uint8_t> b = ((VarsAssignment*)a)->to_bytes();
    memcpy(out, b.data(), b.size());
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
// Are the resident limbs all < q (an assignment made from Montgomery limbs is taken on trust)? report as above; 0 = checked, -1 = error.
int spz_vars_assignment_check_reduced(void* a, uint64_t report[2]) {
  g_err.clear();
  const VarsAssignment* v = (const VarsAssignment*)a;
  const int32_t rc = v && report ? sp_table_check_reduced(v->c, v->tab.h, 0, v->n, report) : SP_EINVAL;
  if (rc != SP_OK) g_err = std::string("spz_vars_assignment_check_reduced: ") + sp_strerror(rc);
  return rc == SP_OK ? 0 : -1;
}
// The same parse for inputs and other short vectors, on the calling thread, no context: limbs_out receives 4 * n Montgomery limbs.
// 0 = ok; -1 with spz_last_error() beginning "InvalidScalar" when an entry is >= q (limbs_out is then not written). report as above.
int spz_scalars_from_bytes(const uint8_t* bytes, size_t n, uint64_t* limbs_out, uint64_t report[2]) {
  return scalar_guard(report, [&]() -> int {
           if ((!bytes || !limbs_out) && n) throw Error("spz_scalars_from_bytes: bad arguments");
           const FqVec v = scalars_from_bytes(bytes, n);
           if (n) memcpy(limbs_out, v[0].l, 32 * n);
           return 1;
         }) == 1 ? 0 : -1;
}
int spz_scalars_to_bytes(const uint64_t* limbs, size_t n, uint8_t* out) {
  try {
    g_err.clear();
    if ((!limbs || !out) && n) throw Error("spz_scalars_to_bytes: bad arguments");
    const std::vector<uint8_t> b = scalars_to_bytes((const sp::Fq*)limbs, n);
    if (n) memcpy(out, b.data(), b.size());
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
// Instance::is_sat (lib.rs:230-259) with the report of the device check: 1 = satisfied, 0 = not, -1 = error (spz_last_error(): "InvalidNumberOfInputs"
// as R1CSError). `assignment` (a spz_vars_assignment_new handle) or `vars` (host scalars). report[0] = violated constraints, report[1] = the first
// (UINT64_MAX when none); rows_out (may be NULL) receives the min(report[0], rows_cap) lowest violated constraint numbers.
int spz_instance_is_sat(void* inst, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs, uint64_t report[2],
                        uint64_t* rows_out, size_t rows_cap) {
  try {
    g_err.clear();
    const Instance& I = *(Instance*)inst;
    SatReport rep;
    const size_t want = rows_out ? rows_cap : 0;
    const bool sat = assignment ? I.is_sat(*(VarsAssignment*)assignment, limbs_vec(inputs, ninputs), &rep, want)
                                : I.is_sat((const sp::Fq*)vars, nvars, limbs_vec(inputs, ninputs), &rep, want);
    if (report) { report[0] = rep.violated; report[1] = rep.first_row; }
    for (size_t i = 0; i < rep.rows.size(); i++) rows_out[i] = rep.rows[i];
    return sat ? 1 : 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
void* spz_snark_prove_resident(void* ctx, void* inst, void* gens, void* enc, void* assignment, const uint64_t* inputs, size_t ninputs,
                               const char* transcript_label, const uint64_t tape_seed[4], double* times10) {
  return guard([&]() -> void* {
    SNARKGens& G = prover_gens<SNARKGens>(gens, "spz_snark_prove_resident");
    Transcript t(transcript_label);
    Fq seed;
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    EncH* e = (EncH*)enc;
    SNARK p = SNARK::prove(*(Ctx*)ctx, *(Instance*)inst, e->comm, e->decomm, *(VarsAssignment*)assignment, limbs_vec(inputs, ninputs), G,
                           t, tape_seed ? &seed : nullptr, &tm);
    fill_times(tm, times10);
    ProofH* h = new ProofH;
    h->bytes = p.serialize();
    return h;
  });
}
void* spz_nizk_prove_resident(void* ctx, void* inst, void* gens, void* assignment, const uint64_t* inputs, size_t ninputs, const char* transcript_label,
                              const uint64_t tape_seed[4], double* times10) {
  return guard([&]() -> void* {
    NIZKGens& G = prover_gens<NIZKGens>(gens, "spz_nizk_prove_resident");
    Transcript t(transcript_label);
    Fq seed;
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    NIZK p = NIZK::prove(*(Ctx*)ctx, *(Instance*)inst, *(VarsAssignment*)assignment, limbs_vec(inputs, ninputs), G, t,
                         tape_seed ? &seed : nullptr, &tm);
    fill_times(tm, times10);
    ProofH* h = new ProofH;
    h->bytes = p.serialize();
    return h;
  });
}
void* spz_nizk_prove(void* ctx, void* inst, void* gens, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                     const char* transcript_label, const uint64_t tape_seed[4], double* times10) {
  return guard([&]() -> void* {
    NIZKGens& G = prover_gens<NIZKGens>(gens, "spz_nizk_prove");
    Transcript t(transcript_label);
    Fq seed;
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    NIZK p = NIZK::prove(*(Ctx*)ctx, *(Instance*)inst, (const sp::Fq*)vars, nvars, limbs_vec(inputs, ninputs), G, t, tape_seed ? &seed : nullptr, &tm);
    fill_times(tm, times10);
    ProofH* h = new ProofH;
    h->bytes = p.serialize();
    return h;
  });
}
// NIZK::verify (lib.rs:549-587) of untrusted proof bytes: 1 accept, 0 reject, -1 malformed bytes (NIZK::deserialize), -2 error (spz_last_error():
// "InvalidNumberOfInputs" as Instance::is_sat raises it, or a device failure). Nothing throws across the boundary.
static int nizk_verify_on(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs, Transcript& t) {
  NIZK p;
  if (!NIZK::deserialize(proof, proof_len, &p)) return -1;
  return p.verify(*(Ctx*)ctx, *(Instance*)inst, limbs_vec(inputs, n_inputs), t, *(NIZKGens*)gens);
}
int spz_nizk_verify(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                    const char* transcript_label) {
  try {
    g_err.clear();
    if (!ctx || !inst || !gens || !proof || !transcript_label || (n_inputs && !inputs)) throw Error("spz_nizk_verify: bad arguments");
    Transcript t(transcript_label);
    return nizk_verify_on(ctx, inst, gens, proof, proof_len, inputs, n_inputs, t);
  } catch (const std::exception& e) {
    g_err = e.what();
    return -2;
  }
}
// the same on a caller-owned transcript (spz_nizk_prove_t): continued by the verification and left in the state it ends in
int spz_nizk_verify_t(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                      uint8_t transcript_state[203]) {
  try {
    g_err.clear();
    if (!ctx || !inst || !gens || !proof || !transcript_state || (n_inputs && !inputs)) throw Error("spz_nizk_verify_t: bad arguments");
    Transcript t(Transcript::FromState(), transcript_state);
    int v = nizk_verify_on(ctx, inst, gens, proof, proof_len, inputs, n_inputs, t);
    t.export_state(transcript_state);
    return v;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -2;
  }
}
// NIZK::verify_many: K untrusted proofs of one instance in lock step on the device (libspartan.hpp), with the return codes of
// spz_snark_verify_many: status_out[k] = 1 accept, 0 reject, -1 malformed bytes and 0 returned; -2 with spz_last_error() for an error of the
// CALL (bad arguments, "InvalidNumberOfInputs" before anything runs, a device failure), status_out then all -2. K = 0 is legal and does nothing.
int spz_nizk_verify_many(void* ctx, void* inst, void* gens, const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* const* inputs,
                         size_t n_inputs, size_t K, const char* transcript_label, int* status_out) {
  try {
    g_err.clear();
    if (!ctx || !inst || !gens || !transcript_label || (K && (!proofs || !proof_lens || !status_out || (n_inputs && !inputs))))
      throw Error("spz_nizk_verify_many: bad arguments");
    for (size_t k = 0; k < K; k++) status_out[k] = -2;
    std::vector<std::pair<const uint8_t*, size_t>> pv(K);
    std::vector<FqVec> in(K);
    std::vector<const FqVec*> inp(K);
    for (size_t k = 0; k < K; k++) {
      if (!proofs[k] || (n_inputs && !inputs[k])) throw Error("spz_nizk_verify_many: bad arguments");
      pv[k] = std::make_pair(proofs[k], proof_lens[k]);
      in[k] = limbs_vec(n_inputs ? inputs[k] : nullptr, n_inputs);
      inp[k] = &in[k];
    }
    std::vector<int> v = NIZK::verify_many(*(Ctx*)ctx, *(Instance*)inst, pv, inp, transcript_label, *(NIZKGens*)gens);
    for (size_t k = 0; k < K; k++) status_out[k] = v[k];
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -2;
  }
}
// test hook (no GPU): parse proof bytes and serialise them again. Returns the number of bytes (written when cap suffices), -1 when malformed.
long long spz_nizk_parse_probe(const uint8_t* proof, size_t len, uint8_t* out, size_t cap) {
  try {
    NIZK p;
    if (!NIZK::deserialize(proof, len, &p)) return -1;
    std::vector<uint8_t> b = p.serialize();
    if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
    return (long long)b.size();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
// ComputationCommitment::deserialize of untrusted bytes (what spz_commitment_bincode writes): the verifier's handle of a circuit, with both share
// vectors uploaded as resident point sets (64 KiB of HBM a share). NULL with spz_last_error() for bytes that are not one commitment, or
// that hold a share that does not decode.
void* spz_commitment_load(void* ctx, const uint8_t* bytes, size_t len) {
  return guard([&]() -> void* {
    if (!ctx || !bytes) throw Error("spz_commitment_load: bad arguments");
    std::unique_ptr<CommH> h(new CommH);
    if (!ComputationCommitment::deserialize(bytes, len, &h->comm)) throw Error("spz_commitment_load: malformed commitment bytes");
    auto upload = [&](const PolyCommitment& pc, sp_points** out) {  // an undecodable share is found here, once (SP_EPOINT)
      int32_t rc = sp_points_upload(((Ctx*)ctx)->h, pc.C[0].data(), pc.C.size(), out);
      if (rc != SP_OK) throw Error(std::string("spz_commitment_load: sp_points_upload failed: ") + sp_strerror(rc));
    };
    upload(h->comm.comm.comm_comb_ops, &h->ops);
    upload(h->comm.comm.comm_comb_mem, &h->mem);
    return h.release();
  });
}
// The same handle computed from the instance itself (SNARK::encode_commitment, libspartan.hpp): the verifier runs the public preprocessing
// instead of trusting bytes. `gens` of either kind — under verifier-only generators the two commitments are sums over the resident point
// sets (verifier.cc) and no window table is ever built. No decommitment is kept. NULL with spz_last_error() on failure.
void* spz_commitment_encode(void* ctx, void* inst, void* gens) {
  return guard([&]() -> void* {
    if (!ctx || !inst || !gens) throw Error("spz_commitment_encode: bad arguments");
    std::unique_ptr<CommH> h(new CommH);
    h->comm = SNARK::encode_commitment(*(Ctx*)ctx, *(Instance*)inst, *(SNARKGens*)gens);
    auto upload = [&](const PolyCommitment& pc, sp_points** out) {
      int32_t rc = sp_points_upload(((Ctx*)ctx)->h, pc.C[0].data(), pc.C.size(), out);
      if (rc != SP_OK) throw Error(std::string("spz_commitment_encode: sp_points_upload failed: ") + sp_strerror(rc));
    };
    upload(h->comm.comm.comm_comb_ops, &h->ops);
    upload(h->comm.comm.comm_comb_mem, &h->mem);
    return h.release();
  });
}
// bincode(ComputationCommitment) of a handle, however it was made: returns the size; fills out when cap suffices
size_t spz_commitment_serialize(void* comm, uint8_t* out, size_t cap) {
  if (!comm) return 0;
  std::vector<uint8_t> b = ((CommH*)comm)->comm.serialize();
  if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
  return b.size();
}
// HBM held by the handle's two resident point sets: 65536 bytes a share
size_t spz_commitment_resident_bytes(void* comm) {
  const CommH* h = (const CommH*)comm;
  return h ? sp_points_table_bytes(h->ops) + sp_points_table_bytes(h->mem) : 0;
}
void spz_commitment_free(void* comm) { delete (CommH*)comm; }
// SNARK::verify (lib.rs:423-466) of untrusted proof bytes against a loaded commitment: 1 accept, 0 reject, -1 malformed bytes (SNARK::deserialize),
// -2 error (spz_last_error(): "InvalidNumberOfInputs", or a device failure). Nothing throws across the boundary.
static int snark_verify_on(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs, Transcript& t) {
  SNARK p;
  if (!SNARK::deserialize(proof, proof_len, &p)) return -1;
  const CommH& h = *(CommH*)comm;
  return p.verify(*(Ctx*)ctx, h.comm, limbs_vec(inputs, n_inputs), t, *(SNARKGens*)gens, ResidentCommitment{h.ops, h.mem});
}
int spz_snark_verify(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                     const char* transcript_label) {
  try {
    g_err.clear();
    if (!ctx || !comm || !gens || !proof || !transcript_label || (n_inputs && !inputs)) throw Error("spz_snark_verify: bad arguments");
    Transcript t(transcript_label);
    return snark_verify_on(ctx, comm, gens, proof, proof_len, inputs, n_inputs, t);
  } catch (const std::exception& e) {
    g_err = e.what();
    return -2;
  }
}
// the same on a caller-owned transcript (spz_snark_prove_t): continued by the verification and left in the state it ends in
int spz_snark_verify_t(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                       uint8_t transcript_state[203]) {
  try {
    g_err.clear();
    if (!ctx || !comm || !gens || !proof || !transcript_state || (n_inputs && !inputs)) throw Error("spz_snark_verify_t: bad arguments");
    Transcript t(Transcript::FromState(), transcript_state);
    int v = snark_verify_on(ctx, comm, gens, proof, proof_len, inputs, n_inputs, t);
    t.export_state(transcript_state);
    return v;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -2;
  }
}
// SNARK::verify_many: K untrusted proofs of one circuit against a loaded commitment, in lock step on the device (libspartan.hpp). Fills
// status_out[k] with 1 accept, 0 reject, -1 malformed bytes and returns 0. Returns -2 with spz_last_error() for an error of the CALL — bad
// arguments, n_inputs that is not the commitment's ("InvalidNumberOfInputs", before anything runs), a device failure, whose text is carried
// over from the worker thread it happened on; status_out is then all -2: nothing is reported as accepted. K = 0 is legal and does nothing.
int spz_snark_verify_many(void* ctx, void* comm, void* gens, const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* const* inputs,
                          size_t n_inputs, size_t K, const char* transcript_label, int* status_out) {
  try {
    g_err.clear();
    if (!ctx || !comm || !gens || !transcript_label || (K && (!proofs || !proof_lens || !status_out || (n_inputs && !inputs))))
      throw Error("spz_snark_verify_many: bad arguments");
    for (size_t k = 0; k < K; k++) status_out[k] = -2;
    std::vector<std::pair<const uint8_t*, size_t>> pv(K);
    std::vector<FqVec> in(K);
    std::vector<const FqVec*> inp(K);
    for (size_t k = 0; k < K; k++) {
      if (!proofs[k] || (n_inputs && !inputs[k])) throw Error("spz_snark_verify_many: bad arguments");
      pv[k] = std::make_pair(proofs[k], proof_lens[k]);
      in[k] = limbs_vec(n_inputs ? inputs[k] : nullptr, n_inputs);
      inp[k] = &in[k];
    }
    const CommH& h = *(CommH*)comm;
    if (K && n_inputs != h.comm.num_inputs) throw Error("InvalidNumberOfInputs");
    std::vector<int> v = SNARK::verify_many(*(Ctx*)ctx, h.comm, pv, inp, transcript_label, *(SNARKGens*)gens, ResidentCommitment{h.ops, h.mem});
    for (size_t k = 0; k < K; k++) status_out[k] = v[k];
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -2;
  }
}
// no GPU, no context: SNARK::deserialize, then SNARK::serialize. Returns the number of bytes (written when cap suffices), -1 when malformed.
long long spz_snark_reserialize(const uint8_t* proof, size_t len, uint8_t* out, size_t cap) {
  try {
    SNARK p;
    if (!SNARK::deserialize(proof, len, &p)) return -1;
    std::vector<uint8_t> b = p.serialize();
    if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
    return (long long)b.size();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
// the same for ComputationCommitment::deserialize / serialize
long long spz_commitment_reserialize(const uint8_t* bytes, size_t len, uint8_t* out, size_t cap) {
  try {
    ComputationCommitment c;
    if (!ComputationCommitment::deserialize(bytes, len, &c)) return -1;
    std::vector<uint8_t> b = c.serialize();
    if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
    return (long long)b.size();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
size_t spz_proof_bytes(void* p, uint8_t* out, size_t cap) {
  ProofH* h = (ProofH*)p;
  if (out && cap >= h->bytes.size()) memcpy(out, h->bytes.data(), h->bytes.size());
  return h->bytes.size();
}
void spz_proof_free(void* p) { delete (ProofH*)p; }

// host-side Fiat–Shamir pieces exposed for CPU tests (no GPU needed)
const char* spz_keccak_variant() { return keccak_f1600_variant(); }
int spz_keccak_run_variant(const char* name, uint64_t state[25]) { return keccak_f1600_run_variant(name, state); }
void spz_shake256(const uint8_t* in, size_t n, uint8_t* out, size_t outlen) { Shake256 s; s.absorb(in, n); s.squeeze(out, outlen); }
size_t spz_merlin_script(const char* tlabel, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas, const size_t* lens,
                         uint8_t* out) {
  Transcript t(tlabel);
  size_t o = 0;
  for (size_t i = 0; i < nops; i++) {
    if (kinds[i] == 0) t.append_message(labels[i], datas[i], lens[i]);
    else if (kinds[i] == 1) { t.challenge_bytes(labels[i], out + o, lens[i]); o += lens[i]; }
    else { uint64_t x; memcpy(&x, datas[i], 8); t.append_u64(labels[i], x); }
  }
  return o;
}
// the 203-byte state of a merlin transcript after `Transcript::new(tlabel)` and a script of messages (kinds as above; no challenges)
void spz_merlin_state(const char* tlabel, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas, const size_t* lens,
                      uint8_t out_state[203]) {
  Transcript t(tlabel);
  uint8_t sink[256];
  for (size_t i = 0; i < nops; i++) {
    if (kinds[i] == 0) t.append_message(labels[i], datas[i], lens[i]);
    else if (kinds[i] == 1) t.challenge_bytes(labels[i], sink, lens[i] < sizeof sink ? lens[i] : sizeof sink);
    else { uint64_t x; memcpy(&x, datas[i], 8); t.append_u64(labels[i], x); }
  }
  t.export_state(out_state);
}
// continue a transcript from a state: one challenge of n bytes (checks import/export round trips in the CPU tests)
void spz_merlin_challenge_from_state(uint8_t state[203], const char* label, uint8_t* out, size_t n) {
  Transcript t(Transcript::FromState(), state);
  t.challenge_bytes(label, out, n);
  t.export_state(state);
}
// The probe of the coarse Rust binding (rust_shim/src/gpu_tail.rs.in, transcript_state / set_transcript_state): that binding reads and writes
// merlin::Transcript's private state through the struct's memory, which `repr(Rust)` does not pin. Before its first use the Rust side runs
// this fixed script on its own merlin transcript — Transcript::new(b"spartan_amd binding probe"), append_message(b"probe-message", 0..63) —
// exports it through the raw copy and compares the 203 bytes with out_state; then it imports out_state into a fresh merlin transcript
// through the raw write and compares challenge_bytes(b"probe-challenge", 32) with out_challenge. A field order or padding that differs
// from {state[200], pos, pos_begin, cur_flags} fails one of the two, in release builds too.
void spz_transcript_probe(uint8_t out_state[203], uint8_t out_challenge[32]) {
  Transcript t("spartan_amd binding probe");
  uint8_t msg[64];
  for (int i = 0; i < 64; i++) msg[i] = (uint8_t)i;
  t.append_message("probe-message", msg, 64);
  t.export_state(out_state);
  t.challenge_bytes("probe-challenge", out_challenge, 32);
}
void spz_tape_draws(const uint64_t seed[4], const char* label, size_t n, uint64_t* out) {
  Fq s;
  memcpy(s.l, seed, 32);
  RandomTape tape("proof", s);
  for (size_t i = 0; i < n; i++) { Fq x = tape.random_scalar(label); memcpy(out + 4 * i, x.l, 32); }
}
}
