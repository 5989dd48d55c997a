// spartan_amd host driver: the C entry points over libspartan.hpp that include/spartan_host.h declares, where each one's contract is written
// down. Exceptions are turned into NULL / error codes and strings here; nothing throws across the boundary.
#include <cstring>
#include <memory>
#include <string>

#include "libspartan.hpp"
#include "fq_inv.hpp"

// an exported function that spartan_host.h (through libspartan.hpp) does not declare, or declares differently, does not compile
#pragma clang diagnostic error "-Wmissing-prototypes"

using namespace spz;

namespace {
thread_local std::string g_err;
struct EncH { ComputationCommitment comm; ComputationDecommitment decomm; };
struct ProofH { std::vector<uint8_t> bytes; };
struct CommH {  // the verifier's handle of a circuit: the commitment and its two share vectors as resident point sets
  ComputationCommitment comm;
  sp_points *ops = nullptr, *mem = nullptr;
  ~CommH() { sp_points_free(ops); sp_points_free(mem); }
  void upload(void* ctx, const char* what) {  // an undecodable share is found here, once (SP_EPOINT)
    const std::pair<const PolyCommitment*, sp_points**> shares[2] = {{&comm.comm.comm_comb_ops, &ops}, {&comm.comm.comm_comb_mem, &mem}};
    for (const auto& s : shares) {
      int32_t rc = sp_points_upload(((Ctx*)ctx)->h, s.first->C[0].data(), s.first->C.size(), s.second);
      if (rc != SP_OK) throw Error(std::string(what) + ": sp_points_upload failed: " + sp_strerror(rc));
    }
  }
};
FqVec limbs_vec(const uint64_t* p, size_t n) { FqVec v(n); if (n) memcpy(v[0].l, p, 32 * n); return v; }
Error bad_arguments(const char* what) { return Error(std::string(what) + ": bad arguments"); }
// the tail of every entry that returns bytes: the size, and the bytes when the caller's buffer holds them
size_t bytes_out(const std::vector<uint8_t>& v, uint8_t* out, size_t cap) {
  if (out && cap >= v.size() && !v.empty()) memcpy(out, v.data(), v.size());
  return v.size();
}
void fill_times(const ProveTimes& t, double* o) {
  if (!o) return;
  o[0] = t.polycommit; o[1] = t.sc_phase_one; o[2] = t.sc_phase_two; o[3] = t.polyeval; o[4] = t.r1cs_sat; o[5] = t.eval_sparse_polys;
  o[6] = t.commit_nondet_witness; o[7] = t.build_layered_network; o[8] = t.evalproof_layered_network; o[9] = t.total;
}
// A generator handle where the PROVER's generators are needed (encode, every prove, the window-table accessors): a verifier-only handle
// is refused here, before any device call — it has no sp_gens, and a null one must never reach a kernel.
template <typename G>
G& prover_gens(void* gens, const char* what) {
  if (!gens) throw bad_arguments(what);
  G& g = *(G*)gens;
  if (g.is_verifier_only()) throw Error(std::string(what) + ": verifier-only generators (they verify; they hold no fixed-base window tables)");
  return g;
}
// The frame of every entry that can fail: the thread's error text is cleared, then f runs; what it throws becomes that text and `fail`.
template <typename R, typename F>
R guard(R fail, F f) {
  try {
    g_err.clear();
    return f();
  } catch (const std::exception& e) {
    g_err = e.what();
    return fail;
  }
}
template <typename F>
void* handle(F f) { return guard((void*)nullptr, f); }
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
// A fresh transcript made from `label`, or, when label is NULL, the caller's own continued from its 203-byte state
Transcript transcript_of(const char* label, const uint8_t* state) { return label ? Transcript(label) : Transcript(Transcript::FromState(), state); }
// Every prove entry. The transcript: `label`, or the caller's `state`, which then receives the state the proof ends in. The assignment: a
// resident handle, read through its table, or host limbs, read in place. prove(vars, n, resident, transcript, seed, times) is SNARK::prove or
// NIZK::prove with the rest of its arguments bound.
template <typename G, typename Prove>
void* prove_entry(const char* what, void* gens, const char* label, uint8_t* state, void* assignment, const uint64_t* vars, size_t nvars,
                  const uint64_t tape_seed[4], double* times10, Prove prove) {
  return handle([&] {
    G& g = prover_gens<G>(gens, what);
    if (!label && (!state || (!assignment && !vars))) throw bad_arguments(what);
    Transcript t = transcript_of(label, state);
    Fq seed;  // tape_seed == NULL: RandomTape::new, seeded from OS entropy (random.rs:13-15)
    if (tape_seed) memcpy(seed.l, tape_seed, 32);
    ProveTimes tm;
    const VarsAssignment* a = (const VarsAssignment*)assignment;
    std::unique_ptr<ProofH> h(new ProofH);
    h->bytes = prove(g, a ? nullptr : (const sp::Fq*)vars, a ? a->n : nvars, a ? a->tab.h : nullptr, t, tape_seed ? &seed : nullptr, &tm).serialize();
    fill_times(tm, times10);
    if (!label) t.export_state(state);
    return h.release();
  });
}
void* snark_prove_entry(const char* what, void* ctx, void* inst, void* gens, void* enc, const char* label, uint8_t* state, void* assignment,
                        const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs, const uint64_t tape_seed[4], double* times10) {
  return prove_entry<SNARKGens>(what, gens, label, state, assignment, vars, nvars, tape_seed, times10,
                                [&](SNARKGens& g, const sp::Fq* v, size_t n, const sp_table* resident, Transcript& t, const Fq* seed, ProveTimes* tm) {
                                  EncH* e = (EncH*)enc;
                                  return SNARK::prove(*(Ctx*)ctx, *(Instance*)inst, e->comm, e->decomm, v, n, limbs_vec(inputs, ninputs), g, t, seed, tm, resident);
                                });
}
void* nizk_prove_entry(const char* what, void* ctx, void* inst, void* gens, const char* label, uint8_t* state, void* assignment, const uint64_t* vars,
                       size_t nvars, const uint64_t* inputs, size_t ninputs, const uint64_t tape_seed[4], double* times10) {
  return prove_entry<NIZKGens>(what, gens, label, state, assignment, vars, nvars, tape_seed, times10,
                               [&](NIZKGens& g, const sp::Fq* v, size_t n, const sp_table* resident, Transcript& t, const Fq* seed, ProveTimes* tm) {
                                 return NIZK::prove(*(Ctx*)ctx, *(Instance*)inst, v, n, limbs_vec(inputs, ninputs), g, t, seed, tm, resident);
                               });
}
// Every verify entry of one proof: the argument check, the transcript as in prove_entry, then verify(transcript) = the verdict
template <typename Verify>
int verify_entry(const char* what, bool args_ok, const char* label, uint8_t* state, Verify verify) {
  return guard(-2, [&] {
    if (!args_ok || (!label && !state)) throw bad_arguments(what);
    Transcript t = transcript_of(label, state);
    int v = verify(t);
    if (!label) t.export_state(state);
    return v;
  });
}
// Both verify_many entries: the caller's K (pointer, length) pairs and K input vectors in the form the library takes them; verify(proofs, inputs) =
// the K verdicts. status_out is all -2 until they are in.
template <typename Verify>
int verify_many_entry(const char* what, bool handles_ok, const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* const* inputs,
                      size_t n_inputs, size_t K, int* status_out, Verify verify) {
  return guard(-2, [&] {
    if (!handles_ok || (K && (!proofs || !proof_lens || !status_out || (n_inputs && !inputs)))) throw bad_arguments(what);
    for (size_t k = 0; k < K; k++) status_out[k] = -2;
    std::vector<std::pair<const uint8_t*, size_t>> pv(K);
    std::vector<FqVec> in(K);
    std::vector<const FqVec*> inp(K);
    for (size_t k = 0; k < K; k++) {
      if (!proofs[k] || (n_inputs && !inputs[k])) throw bad_arguments(what);
      pv[k] = std::make_pair(proofs[k], proof_lens[k]);
      in[k] = limbs_vec(n_inputs ? inputs[k] : nullptr, n_inputs);
      inp[k] = &in[k];
    }
    std::vector<int> v = verify(pv, inp);
    for (size_t k = 0; k < K; k++) status_out[k] = v[k];
    return 0;
  });
}
// the parse-and-serialise-again probes of untrusted bytes, T = SNARK, NIZK or ComputationCommitment
template <typename T>
long long reserialize(const uint8_t* bytes, size_t len, uint8_t* out, size_t cap) {
  return guard(-1LL, [&]() -> long long {
    T x;
    if (!T::deserialize(bytes, len, &x)) return -1;
    return (long long)bytes_out(x.serialize(), out, cap);
  });
}
// the window tables of a prover's generator stream (0: gens_r1cs_sat, 1: gens_r1cs_eval); NULL with the error text for a verifier-only handle
const sp_gens* window_tables_of(void* g, int which, const char* what) {
  return guard((const sp_gens*)nullptr, [&]() -> const sp_gens* {
    SNARKGens& G = prover_gens<SNARKGens>(g, what);
    return which == 0 ? G.stream_sat.g : G.stream_eval.g;
  });
}
// a script of transcript operations (spartan_host.h: spz_merlin_script); challenges go to out back to back, or, when out is NULL, nowhere
size_t merlin_script(Transcript& t, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas, const size_t* lens, uint8_t* out) {
  uint8_t sink[256];
  size_t o = 0;
  for (size_t i = 0; i < nops; i++) {
    if (kinds[i] == 0) t.append_message(labels[i], datas[i], lens[i]);
    else if (kinds[i] == 1 && out) { t.challenge_bytes(labels[i], out + o, lens[i]); o += lens[i]; }
    else if (kinds[i] == 1) t.challenge_bytes(labels[i], sink, lens[i] < sizeof sink ? lens[i] : sizeof sink);
    else { uint64_t x; memcpy(&x, datas[i], 8); t.append_u64(labels[i], x); }
  }
  return o;
}
}  // namespace

extern "C" {
const char* spz_last_error() { return g_err.c_str(); }
void* spz_ctx_new(int device) { return handle([&] { return new Ctx(device); }); }
void spz_ctx_free(void* c) { delete (Ctx*)c; }
sp_ctx* spz_ctx_raw(void* c) { return ((Ctx*)c)->h; }
int spz_ctx_set_option(void* ctx, const char* key, const char* value) { return sp_ctx_set_option(ctx ? ((Ctx*)ctx)->h : nullptr, key, value); }
int spz_ctx_set_commit_shard(void* c, int rank, int world, CommitGatherFn gather, void* user) {
  return guard(-1, [&] { set_commit_shard(*(Ctx*)c, rank, world, gather, user); return 0; });
}
int spz_rccl_unique_id(uint8_t out[128]) { return guard(-1, [&] { rccl_unique_id(out); return 0; }); }
int spz_ctx_set_commit_shard_rccl(void* c, int rank, int world, const uint8_t unique_id[128]) {
  return guard(-1, [&] { set_commit_shard_rccl(*(Ctx*)c, rank, world, unique_id); return 0; });
}
int spz_ctx_set_commit_shard_virtual(void* c, int nshards) { return guard(-1, [&] { set_commit_shard_virtual(*(Ctx*)c, nshards); return 0; }); }
double spz_rccl_allgather_probe(void* c, size_t bytes, int iters) { return guard(-2.0, [&] { return rccl_allgather_probe(((Ctx*)c)->h, bytes, iters); }); }
void spz_ctx_shard_stats(void* c, int reset, uint64_t out[2]) {
  ShardStats s = commit_shard_stats(*(Ctx*)c, reset != 0);
  out[0] = s.gathers; out[1] = s.bytes;
}

void* spz_instance_new(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* rows,
                       const uint64_t* cols, const uint8_t* vals) {
  return handle([&] {
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
        if (!limbs_below_q(raw.l)) throw Error("InvalidScalar");
        e.val = sp::fq_to_mont(raw);
        m[k].push_back(e);
      }
    return new Instance(*(Ctx*)ctx, num_cons, num_vars, num_inputs, m[0], m[1], m[2]);
  });
}
void* spz_instance_from_entries(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* rows,
                                const uint64_t* cols, const uint8_t* vals, int32_t* status, int* matrix, uint64_t report[4]) {
  return entries_guard(status, matrix, report, [&]() -> void* {
    if (!ctx || !nnz) throw bad_arguments("spz_instance_from_entries");
    return Instance::from_entries(*(Ctx*)ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals).release();
  });
}
void* spz_instance_from_device_entries(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, const size_t nnz[3], const uint64_t* const rows[3],
                                       const uint64_t* const cols[3], const uint8_t* const vals[3], int32_t* status, int* matrix, uint64_t report[4]) {
  return entries_guard(status, matrix, report, [&]() -> void* {
    if (!ctx || !nnz || !rows || !cols || !vals) throw bad_arguments("spz_instance_from_device_entries");
    return Instance::from_device_entries(*(Ctx*)ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals).release();
  });
}
void* spz_instance_synthetic(void* ctx, size_t num_cons, size_t num_vars, size_t num_inputs, uint64_t seed, uint64_t* vars_out, uint64_t* inputs_out) {
  return handle([&] {
    FqVec v, in;
    std::unique_ptr<Instance> p = Instance::produce_synthetic_r1cs(*(Ctx*)ctx, num_cons, num_vars, num_inputs, seed, &v, &in);
    if (vars_out) memcpy(vars_out, v[0].l, 32 * v.size());
    if (inputs_out && !in.empty()) memcpy(inputs_out, in[0].l, 32 * in.size());
    return p.release();
  });
}
void spz_instance_free(void* i) { delete (Instance*)i; }
void spz_instance_set_digest(void* inst, const uint8_t* d, size_t n) { ((Instance*)inst)->set_digest(d, n); }
int spz_instance_set_digest_header(void* inst, int old_header) {
  if (((Instance*)inst)->set_digest_header(old_header != 0)) return 0;
  g_err = "set_digest_header after the digest was first used";
  return -1;
}
size_t spz_instance_digest(void* inst, uint8_t* out, size_t cap) {
  return guard((size_t)0, [&] { return bytes_out(((Instance*)inst)->compute_digest(), out, cap); });  // a device failure: 0 and spz_last_error()
}
size_t spz_instance_shape_bincode(void* inst, uint8_t* out, size_t cap) { return bytes_out(((Instance*)inst)->shape_bincode(), out, cap); }
int spz_instance_is_sat(void* inst, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs, uint64_t report[2],
                        uint64_t* rows_out, size_t rows_cap) {
  return guard(-1, [&] {
    const Instance& I = *(Instance*)inst;
    SatReport rep;
    const size_t want = rows_out ? rows_cap : 0;
    const bool sat = assignment ? I.is_sat(*(VarsAssignment*)assignment, limbs_vec(inputs, ninputs), &rep, want)
                                : I.is_sat((const sp::Fq*)vars, nvars, limbs_vec(inputs, ninputs), &rep, want);
    if (report) { report[0] = rep.violated; report[1] = rep.first_row; }
    for (size_t i = 0; i < rep.rows.size(); i++) rows_out[i] = rep.rows[i];
    return sat ? 1 : 0;
  });
}

void* spz_snark_gens_new(void* ctx, size_t nc, size_t nv, size_t ni, size_t nnz) { return handle([&] { return new SNARKGens(*(Ctx*)ctx, nc, nv, ni, nnz); }); }
void* spz_snark_verifier_gens_new(void* ctx, size_t nc, size_t nv, size_t ni, size_t nnz) {
  return handle([&] { return new SNARKGens(SNARKGens::verifier_only(*(Ctx*)ctx, nc, nv, ni, nnz)); });
}
int spz_snark_gens_is_verifier_only(void* g) { return ((SNARKGens*)g)->is_verifier_only() ? 1 : 0; }
size_t spz_snark_gens_resident_bytes(void* g) { return ((SNARKGens*)g)->resident_bytes(); }
void spz_snark_gens_free(void* g) { delete (SNARKGens*)g; }
void* spz_nizk_gens_new(void* ctx, size_t nc, size_t nv, size_t ni) { return handle([&] { return new NIZKGens(*(Ctx*)ctx, nc, nv, ni); }); }
void* spz_nizk_verifier_gens_new(void* ctx, size_t nc, size_t nv, size_t ni) {
  return handle([&] { return new NIZKGens(NIZKGens::verifier_only(*(Ctx*)ctx, nc, nv, ni)); });
}
int spz_nizk_gens_is_verifier_only(void* g) { return ((NIZKGens*)g)->is_verifier_only() ? 1 : 0; }
size_t spz_nizk_gens_resident_bytes(void* g) { return ((NIZKGens*)g)->resident_bytes(); }
void spz_nizk_gens_free(void* g) { delete (NIZKGens*)g; }
size_t spz_snark_gens_stream(void* g, int which, uint8_t* out, size_t cap) {
  return bytes_out(which == 0 ? ((SNARKGens*)g)->stream_sat.compressed : ((SNARKGens*)g)->stream_eval.compressed, out, cap);
}
int spz_snark_gens_window_bits(void* g, int which) { const sp_gens* t = window_tables_of(g, which, "spz_snark_gens_window_bits"); return t ? sp_gens_window_bits(t) : -1; }
int spz_snark_gens_windows(void* g, int which) { const sp_gens* t = window_tables_of(g, which, "spz_snark_gens_windows"); return t ? sp_gens_windows(t) : -1; }
size_t spz_snark_gens_table_bytes(void* g, int which) { const sp_gens* t = window_tables_of(g, which, "spz_snark_gens_table_bytes"); return t ? sp_gens_table_bytes(t) : 0; }
size_t spz_snark_gens_bincode(void* g, uint8_t* out, size_t cap) { return bytes_out(((SNARKGens*)g)->serialize(), out, cap); }

void* spz_snark_encode(void* ctx, void* inst, void* gens) {
  return handle([&] {
    SNARKGens& g = prover_gens<SNARKGens>(gens, "spz_snark_encode");
    std::unique_ptr<EncH> e(new EncH);
    SNARK::encode(*(Ctx*)ctx, *(Instance*)inst, g, &e->comm, &e->decomm);
    return e.release();
  });
}
void spz_encode_free(void* e) { delete (EncH*)e; }
size_t spz_commitment_bincode(void* e, uint8_t* out, size_t cap) { return bytes_out(((EncH*)e)->comm.serialize(), out, cap); }
size_t spz_decommitment_bincode(void* e, uint8_t* out, size_t cap) {
  return guard((size_t)0, [&] { return bytes_out(((EncH*)e)->decomm.serialize(), out, cap); });
}
size_t spz_encode_comm(void* ev, int which, uint8_t* out, size_t cap) {
  EncH* e = (EncH*)ev;
  const PolyCommitment& c = which == 0 ? e->comm.comm.comm_comb_ops : e->comm.comm.comm_comb_mem;
  if (out && cap >= 32 * c.C.size())
    for (size_t i = 0; i < c.C.size(); i++) memcpy(out + 32 * i, c.C[i].data(), 32);
  return c.C.size();
}
void* spz_commitment_load(void* ctx, const uint8_t* bytes, size_t len) {
  return handle([&] {
    if (!ctx || !bytes) throw bad_arguments("spz_commitment_load");
    std::unique_ptr<CommH> h(new CommH);
    if (!ComputationCommitment::deserialize(bytes, len, &h->comm)) throw Error("spz_commitment_load: malformed commitment bytes");
    h->upload(ctx, "spz_commitment_load");
    return h.release();
  });
}
void* spz_commitment_encode(void* ctx, void* inst, void* gens) {
  return handle([&] {
    if (!ctx || !inst || !gens) throw bad_arguments("spz_commitment_encode");
    std::unique_ptr<CommH> h(new CommH);
    h->comm = SNARK::encode_commitment(*(Ctx*)ctx, *(Instance*)inst, *(SNARKGens*)gens);
    h->upload(ctx, "spz_commitment_encode");
    return h.release();
  });
}
size_t spz_commitment_serialize(void* comm, uint8_t* out, size_t cap) { return comm ? bytes_out(((CommH*)comm)->comm.serialize(), out, cap) : 0; }
size_t spz_commitment_resident_bytes(void* comm) {
  const CommH* h = (const CommH*)comm;
  return h ? sp_points_table_bytes(h->ops) + sp_points_table_bytes(h->mem) : 0;
}
void spz_commitment_free(void* comm) { delete (CommH*)comm; }

void* spz_vars_assignment_new(void* ctx, const uint64_t* vars, size_t nvars) {
  return handle([&] { return new VarsAssignment(*(Ctx*)ctx, (const sp::Fq*)vars, nvars); });
}
void spz_vars_assignment_free(void* a) { delete (VarsAssignment*)a; }
void* spz_vars_assignment_from_bytes(void* ctx, const uint8_t* bytes, size_t n, uint64_t report[2]) {
  return scalar_guard(report, [&]() -> void* {
    if (!ctx) throw bad_arguments("spz_vars_assignment_from_bytes");
    return new VarsAssignment(VarsAssignment::from_bytes(*(Ctx*)ctx, bytes, n));
  });
}
void* spz_vars_assignment_from_device_bytes(void* ctx, const uint8_t* dev, size_t n, uint64_t report[2]) {
  return scalar_guard(report, [&]() -> void* {
    if (!ctx) throw bad_arguments("spz_vars_assignment_from_device_bytes");
    return new VarsAssignment(VarsAssignment::from_device_bytes(*(Ctx*)ctx, dev, n));
  });
}
size_t spz_vars_assignment_len(void* a) { return a ? ((VarsAssignment*)a)->n : 0; }
int spz_vars_assignment_to_bytes(void* a, uint8_t* out) {
  return guard(-1, [&] {
    if (!a || !out) throw bad_arguments("spz_vars_assignment_to_bytes");
    const std::vector<uint8_t> b = ((VarsAssignment*)a)->to_bytes();
    memcpy(out, b.data(), b.size());
    return 0;
  });
}
int spz_vars_assignment_check_reduced(void* a, uint64_t report[2]) {
  g_err.clear();
  const VarsAssignment* v = (const VarsAssignment*)a;
  const int32_t rc = v && report ? sp_table_check_reduced(v->c, v->tab.h, 0, v->n, report) : SP_EINVAL;
  if (rc != SP_OK) g_err = std::string("spz_vars_assignment_check_reduced: ") + sp_strerror(rc);
  return rc == SP_OK ? 0 : -1;
}
int spz_scalars_from_bytes(const uint8_t* bytes, size_t n, uint64_t* limbs_out, uint64_t report[2]) {
  return scalar_guard(report, [&]() -> int {
           if ((!bytes || !limbs_out) && n) throw bad_arguments("spz_scalars_from_bytes");
           const FqVec v = scalars_from_bytes(bytes, n);
           if (n) memcpy(limbs_out, v[0].l, 32 * n);
           return 1;
         }) == 1 ? 0 : -1;
}
int spz_scalars_to_bytes(const uint64_t* limbs, size_t n, uint8_t* out) {
  return guard(-1, [&] {
    if ((!limbs || !out) && n) throw bad_arguments("spz_scalars_to_bytes");
    const std::vector<uint8_t> b = scalars_to_bytes((const sp::Fq*)limbs, n);
    if (n) memcpy(out, b.data(), b.size());
    return 0;
  });
}

void* spz_snark_prove(void* ctx, void* inst, void* gens, void* enc, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                      const char* transcript_label, const uint64_t tape_seed[4], double* times10) {
  return snark_prove_entry("spz_snark_prove", ctx, inst, gens, enc, transcript_label, nullptr, nullptr, vars, nvars, inputs, ninputs, tape_seed, times10);
}
void* spz_snark_prove_resident(void* ctx, void* inst, void* gens, void* enc, void* assignment, const uint64_t* inputs, size_t ninputs,
                               const char* transcript_label, const uint64_t tape_seed[4], double* times10) {
  return snark_prove_entry("spz_snark_prove_resident", ctx, inst, gens, enc, transcript_label, nullptr, assignment, nullptr, 0, inputs, ninputs, tape_seed,
                           times10);
}
void* spz_snark_prove_t(void* ctx, void* inst, void* gens, void* enc, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs,
                        size_t ninputs, uint8_t transcript_state[203], const uint64_t tape_seed[4], double* times10) {
  return snark_prove_entry("spz_snark_prove_t", ctx, inst, gens, enc, nullptr, transcript_state, assignment, vars, nvars, inputs, ninputs, tape_seed, times10);
}
void* spz_nizk_prove(void* ctx, void* inst, void* gens, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                     const char* transcript_label, const uint64_t tape_seed[4], double* times10) {
  return nizk_prove_entry("spz_nizk_prove", ctx, inst, gens, transcript_label, nullptr, nullptr, vars, nvars, inputs, ninputs, tape_seed, times10);
}
void* spz_nizk_prove_resident(void* ctx, void* inst, void* gens, void* assignment, const uint64_t* inputs, size_t ninputs, const char* transcript_label,
                              const uint64_t tape_seed[4], double* times10) {
  return nizk_prove_entry("spz_nizk_prove_resident", ctx, inst, gens, transcript_label, nullptr, assignment, nullptr, 0, inputs, ninputs, tape_seed, times10);
}
void* spz_nizk_prove_t(void* ctx, void* inst, void* gens, void* assignment, const uint64_t* vars, size_t nvars, const uint64_t* inputs, size_t ninputs,
                       uint8_t transcript_state[203], const uint64_t tape_seed[4], double* times10) {
  return nizk_prove_entry("spz_nizk_prove_t", ctx, inst, gens, nullptr, transcript_state, assignment, vars, nvars, inputs, ninputs, tape_seed, times10);
}
size_t spz_proof_bytes(void* p, uint8_t* out, size_t cap) { return bytes_out(((ProofH*)p)->bytes, out, cap); }
void spz_proof_free(void* p) { delete (ProofH*)p; }

static int nizk_verify_on(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs, Transcript& t) {
  NIZK p;
  if (!NIZK::deserialize(proof, proof_len, &p)) return -1;
  return p.verify(*(Ctx*)ctx, *(Instance*)inst, limbs_vec(inputs, n_inputs), t, *(NIZKGens*)gens);
}
int spz_nizk_verify(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                    const char* transcript_label) {
  return verify_entry("spz_nizk_verify", ctx && inst && gens && proof && transcript_label && (!n_inputs || inputs), transcript_label, nullptr,
                      [&](Transcript& t) { return nizk_verify_on(ctx, inst, gens, proof, proof_len, inputs, n_inputs, t); });
}
int spz_nizk_verify_t(void* ctx, void* inst, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                      uint8_t transcript_state[203]) {
  return verify_entry("spz_nizk_verify_t", ctx && inst && gens && proof && transcript_state && (!n_inputs || inputs), nullptr, transcript_state,
                      [&](Transcript& t) { return nizk_verify_on(ctx, inst, gens, proof, proof_len, inputs, n_inputs, t); });
}
int spz_nizk_verify_many(void* ctx, void* inst, void* gens, const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* const* inputs,
                         size_t n_inputs, size_t K, const char* transcript_label, int* status_out) {
  return verify_many_entry("spz_nizk_verify_many", ctx && inst && gens && transcript_label, proofs, proof_lens, inputs, n_inputs, K, status_out,
                           [&](const std::vector<std::pair<const uint8_t*, size_t>>& pv, const std::vector<const FqVec*>& inp) {
                             return NIZK::verify_many(*(Ctx*)ctx, *(Instance*)inst, pv, inp, transcript_label, *(NIZKGens*)gens);
                           });
}
static int snark_verify_on(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs, Transcript& t) {
  SNARK p;
  if (!SNARK::deserialize(proof, proof_len, &p)) return -1;
  const CommH& h = *(CommH*)comm;
  return p.verify(*(Ctx*)ctx, h.comm, limbs_vec(inputs, n_inputs), t, *(SNARKGens*)gens, ResidentCommitment{h.ops, h.mem});
}
int spz_snark_verify(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                     const char* transcript_label) {
  return verify_entry("spz_snark_verify", ctx && comm && gens && proof && transcript_label && (!n_inputs || inputs), transcript_label, nullptr,
                      [&](Transcript& t) { return snark_verify_on(ctx, comm, gens, proof, proof_len, inputs, n_inputs, t); });
}
int spz_snark_verify_t(void* ctx, void* comm, void* gens, const uint8_t* proof, size_t proof_len, const uint64_t* inputs, size_t n_inputs,
                       uint8_t transcript_state[203]) {
  return verify_entry("spz_snark_verify_t", ctx && comm && gens && proof && transcript_state && (!n_inputs || inputs), nullptr, transcript_state,
                      [&](Transcript& t) { return snark_verify_on(ctx, comm, gens, proof, proof_len, inputs, n_inputs, t); });
}
int spz_snark_verify_many(void* ctx, void* comm, void* gens, const uint8_t* const* proofs, const size_t* proof_lens, const uint64_t* const* inputs,
                          size_t n_inputs, size_t K, const char* transcript_label, int* status_out) {
  return verify_many_entry("spz_snark_verify_many", ctx && comm && gens && transcript_label, proofs, proof_lens, inputs, n_inputs, K, status_out,
                           [&](const std::vector<std::pair<const uint8_t*, size_t>>& pv, const std::vector<const FqVec*>& inp) {
                             const CommH& h = *(CommH*)comm;
                             if (K && n_inputs != h.comm.num_inputs) throw Error("InvalidNumberOfInputs");
                             return SNARK::verify_many(*(Ctx*)ctx, h.comm, pv, inp, transcript_label, *(SNARKGens*)gens, ResidentCommitment{h.ops, h.mem});
                           });
}

// ---- test hooks ----
long long spz_snark_reserialize(const uint8_t* proof, size_t len, uint8_t* out, size_t cap) { return reserialize<SNARK>(proof, len, out, cap); }
long long spz_nizk_parse_probe(const uint8_t* proof, size_t len, uint8_t* out, size_t cap) { return reserialize<NIZK>(proof, len, out, cap); }
long long spz_commitment_reserialize(const uint8_t* bytes, size_t len, uint8_t* out, size_t cap) { return reserialize<ComputationCommitment>(bytes, len, out, cap); }
size_t spz_zlib_level6(const uint8_t* data, size_t n, int old_header, uint8_t* out, size_t cap) {
  return bytes_out(zlib_level6_miniz(data, n, old_header != 0), out, cap);
}
size_t spz_zlib_probes(const uint8_t* data, size_t n, unsigned probes, int old_header, uint8_t* out, size_t cap) {
  return bytes_out(zlib_miniz_probes(data, n, probes, old_header != 0), out, cap);
}
void spz_deflate_matches_host(const uint8_t* data, size_t n, unsigned probes, uint16_t* L, uint32_t* A, uint32_t* B) {
  if (L) deflate_links_host(data, n, L);
  deflate_matches_host(data, n, probes, L, A, B);
}
size_t spz_zlib_from_matches(const uint8_t* data, size_t n, const uint16_t* L, const uint32_t* A, const uint32_t* B, unsigned probes, int old_header,
                             uint8_t* out, size_t cap, uint64_t stats[2]) {
  uint64_t lookups = 0, fallbacks = 0;
  const std::vector<uint8_t> z = zlib_from_matches(data, n, L, A, B, probes, old_header != 0, &lookups, &fallbacks);
  if (stats) { stats[0] = lookups; stats[1] = fallbacks; }
  return bytes_out(z, out, cap);
}
namespace {
void stats_out(const DeflateStats& s, double* o) {
  if (!o) return;
  const double v[12] = {s.lookups, s.fallbacks, s.segments, s.ms_links, s.ms_search_a, s.ms_search_b, s.ms_download, s.ms_parse, s.ms_wait, s.ms_stream,
                        s.ms_total, s.device};
  memcpy(o, v, sizeof v);
}
}  // namespace
size_t spz_zlib_device(void* ctx, const uint8_t* data, size_t n, unsigned probes, int old_header, uint8_t* out, size_t cap, double stats[12]) {
  return guard((size_t)0, [&] {
    if (!ctx || (n && !data) || probes == 0 || probes > 0xFFF) throw bad_arguments("spz_zlib_device");
    DeflateStats s;
    const std::vector<uint8_t> z = zlib_device(((Ctx*)ctx)->h, data, nullptr, n, probes, old_header != 0, &s, 0);  // this entry is the host parser's
    stats_out(s, stats);
    return bytes_out(z, out, cap);
  });
}
size_t spz_instance_shape_bincode_device(void* inst, uint8_t* out, size_t cap) {
  return guard((size_t)0, [&] { return bytes_out(((Instance*)inst)->shape_bincode_device(), out, cap); });
}
void spz_instance_digest_stats(void* inst, double stats[12]) { stats_out(((Instance*)inst)->digest_stats, stats); }
namespace {
void stats_out_all(const DeflateStats& s, double* o, size_t cap) {
  if (!o) return;
  double v[26];
  stats_out(s, v);
  v[12] = s.parse; v[13] = s.tokens; v[14] = s.device_fallbacks; v[15] = s.ms_reach; v[16] = s.ms_emit;
  v[17] = s.emit; v[18] = s.tokens_coded; v[19] = s.blocks; v[20] = s.stored_blocks; v[21] = s.static_blocks; v[22] = s.ms_blocks; v[23] = s.ms_bits;
  v[24] = s.ms_tables; v[25] = s.ms_bytes;
  memcpy(o, v, sizeof(double) * std::min<size_t>(cap, 26));
}
}  // namespace
size_t spz_deflate_tokens_host(const uint8_t* data, size_t n, unsigned probes, const size_t* geom, uint32_t* tokens, uint64_t* counters) {
  return deflate_tokens_host(data, n, probes, geom, tokens, counters);
}
size_t spz_zlib_from_tokens(const uint8_t* data, size_t n, const uint32_t* tokens, size_t ntok, unsigned probes, int old_header, size_t piece,
                            uint8_t* out, size_t cap, uint64_t* blocks) {
  return bytes_out(zlib_from_tokens(data, n, tokens, ntok, probes, old_header != 0, piece, blocks), out, cap);
}
size_t spz_zlib_device_parse(void* ctx, const uint8_t* data, size_t n, unsigned probes, int old_header, int parse, size_t tile, size_t group,
                             uint8_t* out, size_t cap, double* stats, size_t stats_cap) {
  return guard((size_t)0, [&] {
    if (!ctx || (n && !data) || probes == 0 || probes > 0xFFF || parse < -1 || parse > 1) throw bad_arguments("spz_zlib_device_parse");
    DeflateStats s;
    const std::vector<uint8_t> z = zlib_device(((Ctx*)ctx)->h, data, nullptr, n, probes, old_header != 0, &s, parse, tile, group);
    stats_out_all(s, stats, stats_cap);
    return bytes_out(z, out, cap);
  });
}
size_t spz_zlib_device_emit(void* ctx, const uint8_t* data, size_t n, unsigned probes, int old_header, int parse, size_t tile, size_t group, size_t chunk,
                            uint8_t* out, size_t cap, double* stats, size_t stats_cap) {
  return guard((size_t)0, [&] {
    if (!ctx || (n && !data) || probes == 0 || probes > 0xFFF || parse < -1 || parse > 2) throw bad_arguments("spz_zlib_device_emit");
    DeflateStats s;
    const std::vector<uint8_t> z = zlib_device(((Ctx*)ctx)->h, data, nullptr, n, probes, old_header != 0, &s, parse, tile, group, chunk);
    stats_out_all(s, stats, stats_cap);
    return bytes_out(z, out, cap);
  });
}
long long spz_deflate_blocks_host(const uint32_t* tokens, size_t ntok, size_t n, size_t segment, uint64_t* records, uint16_t* hist, size_t cap,
                                  uint64_t* counters) {
  return guard((long long)-1, [&] { return (long long)deflate_blocks_host(tokens, ntok, n, segment, records, hist, cap, counters); });
}
size_t spz_zlib_from_blocks(const uint64_t* records, const uint16_t* hist, size_t nblocks, const uint32_t* tokens, const uint8_t* data, size_t n,
                            unsigned probes, int old_header, uint8_t* out, size_t cap, uint64_t* stats) {
  return guard((size_t)0, [&] { return bytes_out(zlib_from_blocks(records, hist, nblocks, tokens, data, n, probes, old_header != 0, stats), out, cap); });
}
void spz_instance_digest_stats_all(void* inst, double* stats, size_t stats_cap) { stats_out_all(((Instance*)inst)->digest_stats, stats, stats_cap); }
const char* spz_keccak_variant() { return keccak_f1600_variant(); }
int spz_keccak_run_variant(const char* name, uint64_t state[25]) { return keccak_f1600_run_variant(name, state); }
void spz_shake256(const uint8_t* in, size_t n, uint8_t* out, size_t outlen) { Shake256 s; s.absorb(in, n); s.squeeze(out, outlen); }
size_t spz_merlin_script(const char* tlabel, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas, const size_t* lens,
                         uint8_t* out) {
  Transcript t(tlabel);
  return merlin_script(t, nops, kinds, labels, datas, lens, out);
}
void spz_merlin_state(const char* tlabel, size_t nops, const int* kinds, const char* const* labels, const uint8_t* const* datas, const size_t* lens,
                      uint8_t out_state[203]) {
  Transcript t(tlabel);
  merlin_script(t, nops, kinds, labels, datas, lens, nullptr);
  t.export_state(out_state);
}
void spz_merlin_challenge_from_state(uint8_t state[203], const char* label, uint8_t* out, size_t n) {
  Transcript t(Transcript::FromState(), state);
  t.challenge_bytes(label, out, n);
  t.export_state(state);
}
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
void spz_seed_scalar(const char* domain, uint64_t seed, uint64_t out[4]) { Fq s = seed_scalar(domain, seed); memcpy(out, s.l, 32); }
void spz_fq_invert_vartime(const uint64_t in[4], uint64_t out[4]) { Fq a; memcpy(a.l, in, 32); Fq r = fq_invert_vartime(a); memcpy(out, r.l, 32); }
int spz_unipoly_probe(const uint64_t* evals, size_t n, const uint64_t r[4], uint64_t* coeffs, uint64_t* compressed, uint64_t eval_at_r[4]) {
  return guard(-1, [&] {
    FqVec c, cc;
    Fq rr, ev;
    memcpy(rr.l, r, 32);
    unipoly_probe(limbs_vec(evals, n), rr, &c, &cc, &ev);
    memcpy(coeffs, c.data(), 32 * c.size());
    memcpy(compressed, cc.data(), 32 * cc.size());
    memcpy(eval_at_r, ev.l, 32);
    return 0;
  });
}
void spz_cubic_coeffs_probe(const uint64_t S[48], const uint64_t r[4], uint64_t ev[12]) {
  Fq s[12], rr, e[3];
  memcpy(s, S, sizeof s); memcpy(rr.l, r, 32);
  cubic_coeffs_probe(s, rr, e);
  memcpy(ev, e, sizeof e);
}
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
  FqVec evc, K;
  if (!eq_factor_probe(limbs_vec(rho, nvars), np, ni, limbs_vec(coeffs, ni), limbs_vec(claims, nrounds), limbs_vec(ev4, 4 * ni * nrounds),
                       limbs_vec(challenges, nrounds), &evc, &K))
    return 0;
  memcpy(evc_out, evc.data(), 32 * evc.size());
  memcpy(K_out, K.data(), 32 * K.size());
  return 1;
}
}
