// spartan_amd host driver: NIZK::verify and SNARK::verify of libspartan (src/lib.rs:549-587, 423-466) and the sub-verifiers under them, over the C ABI.
// Where each piece runs:
//   R1CSInstance::evaluate(rx, ry)  NIZK: device: sp_eq_expand x 2, sp_sparse_evaluate_begin on the instance's resident matrices, collected with
//                                   sp_job_wait when R1CSProof::verify needs the three values (the kernels run under the host's Sigma protocols).
//                                   NIZK::verify_many: ONE sp_sparse_evaluate_many_begin for the batch, at every proof's own point
//                                   SNARK: the three values the proof claims; the sparse-polynomial evaluation proof binds them to the commitment
//   C_LZ = <L, comm.C>              device. Points that arrive with the proof (comm_vars; the SNARK's comm_derefs): sp_msm_var. The two commitments
//                                   of a ComputationCommitment, fixed for a circuit: sp_msm_points over their resident point sets (sp_points) when
//                                   the caller holds them, else sp_msm_var as well. polyeval_verify is the one place that chooses
//   G_hat = <s, G>                  device: sp_commit_rows, one row over the fixed-base tables of gens_n; under VERIFIER-ONLY generators
//                                   (GensStream::verifier_only, below: a stream is a resident point set there and no sp_gens exists)          
//                                   sp_msm_points_range over gens_n's range of the stream's set. dev_commit_row is the one place that chooses
//   the circuit's commitment        SNARK::encode_commitment (below): the dense representation of the prover's encode, then comb_ops and comb_mem
//                                   committed over the window tables (poly_commit) or, under verifier-only generators, over gens_n's range of the
//                                   stream's resident set: sp_commit_rows_points, one call a polynomial. No decommitment is kept
//   everything with <= 64 terms     calling thread: sp_host_msm_var (proof points, generators by their encodings), sp_host_commit_small when
//                                   every base is a generator (sp_host_commit_small_points under verifier-only generators: commit_gens)
//   the SPARK sum-checks            calling thread: field arithmetic over the proof's scalars and the transcript, no groups (SumcheckInstanceProof,
//                                   ProductCircuitEvalProofBatched, ProductLayerProof, HashLayerProof::verify_helper)
//   point equalities                comparisons of 32-byte encodings
// SNARK::verify_many (at the end of the file) runs K of these verifications on K threads; their C_LZ and G_hat calls then meet at a gate
// (batch_gate.hpp) and go out once per batch: sp_msm_var_many, sp_msm_points_range_many, sp_commit_rows with K rows. NIZK::verify_many does the same
// for NIZK::verify, whose third device request, the evaluation of the instance, becomes one job of the batch.
// Verdicts: 1 accept, 0 reject, -1 malformed bytes. The input is untrusted: where the reference panics on attacker-controlled data
// (decompress().unwrap() at dense_mlpoly.rs:382, r1csproof.rs:409, nizk/mod.rs:239; the length asserts of sumcheck.rs:38,44,97-98, nizk/mod.rs:381,
// 536-537, product_tree.rs:395,417-418,425, sparse_mlpoly.rs:167,861-883,910,922-930,1238-1268,1379-1381,1531 and the slice indices next to
// them; assert_eq!(rx, claimed_rx) at lib.rs:580-581) this returns 0. r1cs_verify takes the three evaluations from its caller, as
// R1CSProof::verify does (r1csproof.rs:351-359): NIZK::verify computes them, SNARK::verify hands over the proof's.
#include "libspartan.hpp"
#include "batch_gate.hpp"
#include "fq_inv.hpp"

#include <algorithm>
#include <functional>
#include <thread>

namespace spz {
using namespace sp;

namespace {
struct Reject {};  // a check of the protocol failed, or a point of the proof does not decode: verdict 0

Error dev_error(const char* what, int32_t rc) { return Error(std::string(what) + " failed: " + sp_strerror(rc) + " (" + std::to_string(rc) + ")"); }
void spx(int32_t rc, const char* what) {
  if (rc == SP_EPOINT) throw Reject();
  if (rc != SP_OK) throw dev_error(what, rc);
}
void require(bool cond) { if (!cond) throw Reject(); }
const uint64_t* U(const FqVec& v) { return v.empty() ? nullptr : v[0].l; }
size_t log_2(size_t n) {  // math.rs:21-29
  size_t l = 0;
  while (((size_t)1 << l) < n) l++;
  return l;
}
FqVec eq_evals(const Fq* r, size_t ell) {  // EqPolynomial::evals (dense_mlpoly.rs:68-84) for the sqrt(N)-sized L and R
  FqVec evals((size_t)1 << ell, fq_one());
  size_t size = 1;
  for (size_t j = 0; j < ell; j++) {
    size *= 2;
    for (size_t i = size - 1;; i -= 2) {
      Fq scalar = evals[i / 2];
      evals[i] = scalar * r[j];
      evals[i - 1] = scalar - evals[i];
      if (i == 1) break;
    }
  }
  return evals;
}
Fq dot(const FqVec& a, const FqVec& b) {
  Fq s = fq_zero();
  for (size_t i = 0; i < a.size(); i++) s += a[i] * b[i];
  return s;
}
const CP kIdentity{};  // the encoding of the identity: 32 zero bytes

// sum_k s[k] * P[k] over at most 64 encoded points on this core (GroupElement::vartime_multiscalar_mul and the a * P + Q forms of the verifiers)
struct Terms {
  std::vector<uint8_t> pts;
  FqVec s;
  Terms& add(const uint8_t* p, const Fq& k) { pts.insert(pts.end(), p, p + 32); s.push_back(k); return *this; }
  Terms& add(const CP& p, const Fq& k) { return add(p.data(), k); }
  CP eval() const {
    CP out;
    spx(sp_host_msm_var(pts.data(), U(s), s.size(), out.data()), "sp_host_msm_var");
    return out;
  }
};
// the generators of one SHAKE stream by their encodings (GensStream::compressed), for the combinations that mix them with proof points
struct GenBytes {
  const std::vector<uint8_t>& comp;
  const uint8_t* at(uint32_t idx) const { return comp.data() + 32 * (size_t)idx; }
};
// sum_k s[k] * P[idx[k]] over generators only (Scalar::commit / [Scalar]::commit, commitments.rs:73-92)
// over the host window tables of the stream's set, whichever kind of set the generators hold
CP commit_gens(const MultiCommitGens& g, const std::vector<uint32_t>& idx, const FqVec& s) {
  CP out;
  if (g.g) spx(sp_host_commit_small(g.g, idx.data(), idx.size(), U(s), 1, nullptr, out.data()), "sp_host_commit_small");
  else spx(sp_host_commit_small_points(g.p, idx.data(), idx.size(), U(s), 1, nullptr, out.data()), "sp_host_commit_small_points");
  return out;
}

// ---- the three blocking device calls of a verification. A verification run by SNARK::verify_many has a gate (batch_gate.hpp) on its thread:
// the call is then POSTED there and answered by the batch's leader, who issues one device call for all the requests of the same shape. Without
// a gate (every single-proof verifier) the call goes straight to the device. Requests that may share a call have equal keys:
//   (var, n)                     sp_msm_var over n points of the proof        -> sp_msm_var_many
//   (points, set, g_off, n)      sp_msm_points[_range] over a resident set    -> sp_msm_points_range_many
//   (rows, gens, g_off, h, n)    sp_commit_rows of one unblinded row          -> sp_commit_rows with rows = the group's size
//   (eval_start, instance)       R1CSInstance::evaluate at (rx, ry), started  -> sp_sparse_evaluate_many_begin, one job for the group
//   (eval_collect, instance)     ... its three values                         -> sp_job_wait, once (NIZK::verify_many only)
struct DevKey {
  enum Kind { VAR, POINTS, ROWS, EVAL_START, EVAL_COLLECT } kind;
  const void* obj;  // the sp_points, the sp_gens or the Instance; null for VAR
  size_t g_off, h, n;
  bool operator<(const DevKey& o) const {
    if (kind != o.kind) return kind < o.kind;
    if (obj != o.obj) return std::less<const void*>()(obj, o.obj);
    if (g_off != o.g_off) return g_off < o.g_off;
    if (h != o.h) return h < o.h;
    return n < o.n;
  }
};
struct DevReq { const uint8_t* points; const uint64_t* S; const uint64_t* S2 = nullptr; };  // n encodings (VAR only) and n scalars, alive while the member waits; EVAL_START: S = rx, S2 = ry
struct DevAns { int32_t rc = SP_OK; CP out{}; uint64_t ev[12] = {0}; };  // ev: EVAL_COLLECT's (A, B, C)(rx, ry)
typedef BatchGate<DevKey, DevReq, DevAns> VerifyGate;
struct GateSeat { VerifyGate* gate = nullptr; size_t member = 0; };
thread_local GateSeat tl_seat;  // set by a worker thread of verify_many for its lifetime; null on every other thread

void dev_answer(const DevKey& key, const DevReq& req, uint8_t out[32], const char* what) {
  DevAns a = tl_seat.gate->post(tl_seat.member, key, req);
  spx(a.rc, what);
  memcpy(out, a.out.data(), 32);
}
void dev_msm_var(sp_ctx* c, const uint8_t* points, const uint64_t* S, size_t n, uint8_t out[32]) {
  if (!tl_seat.gate) spx(sp_msm_var(c, points, S, n, out), "sp_msm_var");
  else dev_answer(DevKey{DevKey::VAR, nullptr, 0, 0, n}, DevReq{points, S}, out, "sp_msm_var_many");
}
void dev_msm_points(sp_ctx* c, const sp_points* set, const uint64_t* S, size_t n, uint8_t out[32]) {
  if (!tl_seat.gate) spx(sp_msm_points(c, set, S, n, out), "sp_msm_points");  // SP_EINVAL for another size cannot happen: the caller required it
  else dev_answer(DevKey{DevKey::POINTS, set, 0, 0, n}, DevReq{nullptr, S}, out, "sp_msm_points_range_many");
}
// <S, gn.G>, one unblinded row over the n generators of gn (consecutive in their stream): the fixed-base tables of the prover's generators, or
// that range of the resident set of verifier-only ones
void dev_commit_row(sp_ctx* c, const MultiCommitGens& gn, const uint64_t* S, size_t n, uint8_t out[32]) {
  const size_t g_off = gn.G[0];
  if (gn.g) {
    if (!tl_seat.gate) spx(sp_commit_rows(c, gn.g, g_off, gn.h, S, 1, n, nullptr, out), "sp_commit_rows");
    else dev_answer(DevKey{DevKey::ROWS, gn.g, g_off, gn.h, n}, DevReq{nullptr, S}, out, "sp_commit_rows");
  } else {
    if (!tl_seat.gate) spx(sp_msm_points_range(c, gn.p, g_off, n, S, out), "sp_msm_points_range");
    else dev_answer(DevKey{DevKey::POINTS, gn.p, g_off, 0, n}, DevReq{nullptr, S}, out, "sp_msm_points_range_many");
  }
}

// ---- nizk/mod.rs ----
void knowledge_verify(const KnowledgeProof& p, const MultiCommitGens& g, Transcript& t, const CP& C) {  // :54-75
  t.append_protocol_name("knowledge proof");
  t.append_point("C", C.data());
  t.append_point("alpha", p.alpha.data());
  Fq c = t.challenge_scalar("c");
  CP lhs = commit_gens(g, {g.G[0], g.h}, {p.z1, p.z2});
  CP rhs = Terms().add(C, c).add(p.alpha, fq_one()).eval();
  require(lhs == rhs);
}
void equality_verify(const EqualityProof& p, const MultiCommitGens& g, Transcript& t, const CP& C1, const CP& C2) {  // :118-143
  t.append_protocol_name("equality proof");
  t.append_point("C1", C1.data());
  t.append_point("C2", C2.data());
  t.append_point("alpha", p.alpha.data());
  Fq c = t.challenge_scalar("c");
  CP rhs = Terms().add(C1, c).add(C2, -c).add(p.alpha, fq_one()).eval();  // c (C1 - C2) + alpha
  CP lhs = commit_gens(g, {g.h}, {p.z});
  require(lhs == rhs);
}
void product_verify(const ProductProof& p, const MultiCommitGens& g, const GenBytes& gb, Transcript& t, const CP& X, const CP& Y, const CP& Z) {  // :245-289
  t.append_protocol_name("product proof");
  t.append_point("X", X.data());
  t.append_point("Y", Y.data());
  t.append_point("Z", Z.data());
  t.append_point("alpha", p.alpha.data());
  t.append_point("beta", p.beta.data());
  t.append_point("delta", p.delta.data());
  Fq c = t.challenge_scalar("c");
  // check_equality (:231-243): P + c X == commit(z1, z2)
  require(Terms().add(p.alpha, fq_one()).add(X, c).eval() == commit_gens(g, {g.G[0], g.h}, {p.z[0], p.z[1]}));
  require(Terms().add(p.beta, fq_one()).add(Y, c).eval() == commit_gens(g, {g.G[0], g.h}, {p.z[2], p.z[3]}));
  // the third under {G: X, h}: delta + c Z == z3 X + z5 h
  require(Terms().add(p.delta, fq_one()).add(Z, c).eval() == Terms().add(X, p.z[2]).add(gb.at(g.h), p.z[4]).eval());
}
void dotproduct_verify(const DotProductProof& p, const MultiCommitGens& g1, const MultiCommitGens& gn, Transcript& t, const FqVec& a, const CP& Cx,
                       const CP& Cy) {  // :372-404
  require(gn.n() == a.size() && g1.n() == 1 && p.z.size() == a.size());
  t.append_protocol_name("dot product proof");
  t.append_point("Cx", Cx.data());
  t.append_point("Cy", Cy.data());
  t.append_scalars("a", a);
  t.append_point("delta", p.delta.data());
  t.append_point("beta", p.beta.data());
  Fq c = t.challenge_scalar("c");
  std::vector<uint32_t> idx(gn.G);
  idx.push_back(gn.h);
  FqVec zs(p.z);
  zs.push_back(p.z_delta);
  bool ok = Terms().add(Cx, c).add(p.delta, fq_one()).eval() == commit_gens(gn, idx, zs);
  ok &= Terms().add(Cy, c).add(p.beta, fq_one()).eval() == commit_gens(g1, {g1.G[0], g1.h}, {dot(p.z, a), p.z_beta});
  require(ok);
}
// BulletReductionProof::verify with verification_scalars (bullet.rs:137-225). Gamma = Cx + r Cy is folded into the Gamma_hat combination.
void bullet_verify(sp_ctx* c, const BulletReductionProof& p, size_t n, const FqVec& a, Transcript& t, const CP& Cx, const CP& Cy, const Fq& r,
                   const MultiCommitGens& gn, CP* g_hat, CP* Gamma_hat, Fq* a_hat) {
  const size_t lg_n = p.L_vec.size();
  require(lg_n < 32);                                          // :143-147
  require(n == ((size_t)1 << lg_n));                           // :148-150
  require(p.R_vec.size() == lg_n && gn.n() == n && a.size() == n);
  FqVec u(lg_n);
  for (size_t i = 0; i < lg_n; i++) {                          // :154-158
    t.append_point("L", p.L_vec[i].data());
    t.append_point("R", p.R_vec[i].data());
    u[i] = t.challenge_scalar("u");
  }
  FqVec u_inv(lg_n);                                           // :161-162 batch_invert: the inverses and their product
  Fq allinv = fq_one();
  for (size_t i = 0; i < lg_n; i++) { u_inv[i] = fq_invert_vartime(u[i]); allinv *= u_inv[i]; }
  FqVec u_sq(lg_n), u_inv_sq(lg_n);
  for (size_t i = 0; i < lg_n; i++) { u_sq[i] = u[i] * u[i]; u_inv_sq[i] = u_inv[i] * u_inv[i]; }
  FqVec s(n);                                                  // :173-182
  s[0] = allinv;
  for (size_t i = 1; i < n; i++) {
    size_t lg_i = 0;
    while (((size_t)2 << lg_i) <= i) lg_i++;
    s[i] = s[i - ((size_t)1 << lg_i)] * u_sq[(lg_n - 1) - lg_i];
  }
  // G_hat = <s, G> (:213): fixed bases, the device's window tables (verifier-only generators: that range of the stream's resident set)
  dev_commit_row(c, gn, U(s), n, g_hat->data());
  *a_hat = dot(a, s);                                          // :214
  Terms g;                                                     // :216-222
  for (size_t i = 0; i < lg_n; i++) g.add(p.L_vec[i], u_sq[i]);
  for (size_t i = 0; i < lg_n; i++) g.add(p.R_vec[i], u_inv_sq[i]);
  g.add(Cx, fq_one()).add(Cy, r);
  *Gamma_hat = g.eval();
}
void dotproductlog_verify(sp_ctx* c, const DotProductProofLog& p, size_t n, const DotProductProofGens& gens, const GenBytes& gb, Transcript& t, const FqVec& a,
                          const CP& Cx, const CP& Cy) {  // nizk/mod.rs:527-577
  require(gens.n == n && a.size() == n);
  t.append_protocol_name("dot product proof (log)");
  t.append_point("Cx", Cx.data());
  t.append_point("Cy", Cy.data());
  t.append_scalars("a", a);
  Fq r = t.challenge_scalar("r");  // gens_1_scaled = {G: r gens_1.G, h}
  CP g_hat, Gamma_hat;
  Fq a_hat;
  bullet_verify(c, p.bullet, n, a, t, Cx, Cy, r, gens.gens_n, &g_hat, &Gamma_hat, &a_hat);
  t.append_point("delta", p.delta.data());
  t.append_point("beta", p.beta.data());
  Fq ch = t.challenge_scalar("c");
  // lhs = (Gamma_hat c + beta) a_hat + delta ; rhs = (g_hat + r a_hat G_1) z1 + z2 h
  CP lhs = Terms().add(Gamma_hat, ch * a_hat).add(p.beta, a_hat).add(p.delta, fq_one()).eval();
  CP rhs = Terms().add(g_hat, p.z1).add(gb.at(gens.gens_1.G[0]), r * a_hat * p.z1).add(gb.at(gens.gens_1.h), p.z2).eval();
  require(lhs == rhs);
}
// PolyEvalProof::verify (dense_mlpoly.rs:367-389)
void polyeval_verify(sp_ctx* c, const PolyEvalProof& p, const PolyCommitmentGens& gens, const GenBytes& gb, Transcript& t, const Fq* r, size_t ell,
                     const CP& C_Zr, const PolyCommitment& comm, const sp_points* resident = nullptr /* comm.C as a resident point set, when one exists */) {
  t.append_protocol_name("polynomial evaluation proof");
  const size_t left = ell / 2;  // compute_factored_lens (:86-88)
  // before anything of that size is expanded: ell follows from vector lengths of the proof, the commitment and the generators do not
  require(left < 32 && comm.C.size() == (size_t)1 << left && gens.gens.n == (size_t)1 << (ell - left));
  require(!resident || sp_points_count(resident) == comm.C.size());
  FqVec L = eq_evals(r, left), R = eq_evals(r + left, ell - left);
  CP C_LZ;  // :382-384, over the commitment shares the proof carries
  static_assert(sizeof(CP) == 32, "CP is 32 packed bytes");
  if (resident) dev_msm_points(c, resident, U(L), L.size(), C_LZ.data());
  else dev_msm_var(c, comm.C[0].data(), U(L), L.size(), C_LZ.data());
  dotproductlog_verify(c, p.proof, R.size(), gens.gens, gb, t, R, C_LZ, C_Zr);
}
// ZKSumcheckInstanceProof::verify (sumcheck.rs:84-179)
CP zk_sumcheck_verify(const ZKSumcheckInstanceProof& p, const CP& comm_claim, size_t num_rounds, size_t degree_bound, const MultiCommitGens& g1,
                      const MultiCommitGens& gn, Transcript& t, FqVec* r_out) {
  require(gn.n() == degree_bound + 1);
  require(p.comm_polys.size() == num_rounds && p.comm_evals.size() == num_rounds && p.proofs.size() == num_rounds && num_rounds > 0);
  FqVec r;
  for (size_t i = 0; i < num_rounds; i++) {
    t.append_point("comm_poly", p.comm_polys[i].data());
    Fq r_i = t.challenge_scalar("challenge_nextround");
    const CP& claim = i == 0 ? comm_claim : p.comm_evals[i - 1];
    const CP& comm_eval = p.comm_evals[i];
    t.append_point("comm_claim_per_round", claim.data());
    t.append_point("comm_eval", comm_eval.data());
    FqVec w = t.challenge_vector("combine_two_claims_to_one", 2);
    CP comm_target = Terms().add(claim, w[0]).add(comm_eval, w[1]).eval();  // :127-134
    FqVec a(degree_bound + 1);
    Fq pw = fq_one();
    for (size_t j = 0; j <= degree_bound; j++) {  // w0 * (2, 1, 1, ..) + w1 * (1, r, r^2, ..)
      a[j] = w[0] * (j == 0 ? fq_one() + fq_one() : fq_one()) + w[1] * pw;
      pw *= r_i;
    }
    dotproduct_verify(p.proofs[i], g1, gn, t, a, p.comm_polys[i], comm_target);
    r.push_back(r_i);
  }
  *r_out = r;
  return p.comm_evals.back();
}
// R1CSProof::verify (r1csproof.rs:351-490). `evals` yields (A, B, C)(rx, ry) when the last check needs them: NIZK::verify computes them on the
// device meanwhile; SNARK::verify hands over the values its proof claims.
typedef std::function<void(Fq out[3])> EvalsFn;
void r1cs_verify(sp_ctx* c, const R1CSProof& P, size_t num_vars, size_t num_cons, const FqVec& input, const EvalsFn& evals, Transcript& t,
                 const R1CSGens& gens, const GenBytes& gb, FqVec* rx_out, FqVec* ry_out) {
  t.append_protocol_name("R1CS proof");
  t.append_scalars("input", input);
  t.append_message("poly_commitment", "poly_commitment_begin");  // dense_mlpoly.rs:292-300
  for (auto& pt : P.comm_vars.C) t.append_point("poly_commitment_share", pt.data());
  t.append_message("poly_commitment", "poly_commitment_end");
  const size_t num_rounds_x = log_2(num_cons), num_rounds_y = log_2(2 * num_vars);
  FqVec tau = t.challenge_vector("challenge_tau", num_rounds_x);
  const MultiCommitGens& g1 = gens.gens_sc.gens_1;
  FqVec rx, ry;
  CP comm_claim_post_phase1 = zk_sumcheck_verify(P.sc_proof_phase1, kIdentity /* commit(0, 0) */, num_rounds_x, 3, g1, gens.gens_sc.gens_4, t, &rx);
  const CP &comm_Az = P.claims_phase2[0], &comm_Bz = P.claims_phase2[1], &comm_Cz = P.claims_phase2[2], &comm_prod = P.claims_phase2[3];
  knowledge_verify(P.pok_claims_phase2, g1, t, comm_Cz);
  product_verify(P.proof_prod, g1, gb, t, comm_Az, comm_Bz, comm_prod);
  t.append_point("comm_Az_claim", comm_Az.data());
  t.append_point("comm_Bz_claim", comm_Bz.data());
  t.append_point("comm_Cz_claim", comm_Cz.data());
  t.append_point("comm_prod_Az_Bz_claims", comm_prod.data());
  Fq taus_bound_rx = fq_one();
  for (size_t i = 0; i < rx.size(); i++) taus_bound_rx *= rx[i] * tau[i] + (fq_one() - rx[i]) * (fq_one() - tau[i]);
  CP expected_post1 = Terms().add(comm_prod, taus_bound_rx).add(comm_Cz, -taus_bound_rx).eval();  // :408-410
  equality_verify(P.proof_eq_sc_phase1, g1, t, expected_post1, comm_claim_post_phase1);
  Fq r_A = t.challenge_scalar("challenge_Az"), r_B = t.challenge_scalar("challenge_Bz"), r_C = t.challenge_scalar("challenge_Cz");
  CP comm_claim_phase2 = Terms().add(comm_Az, r_A).add(comm_Bz, r_B).add(comm_Cz, r_C).eval();  // :426-436
  CP comm_claim_post_phase2 = zk_sumcheck_verify(P.sc_proof_phase2, comm_claim_phase2, num_rounds_y, 2, g1, gens.gens_sc.gens_3, t, &ry);
  polyeval_verify(c, P.proof_eval_vars_at_ry, gens.gens_pc, gb, t, ry.data() + 1, ry.size() - 1, P.comm_vars_at_ry, P.comm_vars);
  // SparsePolynomial::evaluate of (1, input) at ry[1..] (:457-467, sparse_mlpoly.rs:1576-1592)
  const size_t nv = log_2(num_vars);
  require(nv == ry.size() - 1);
  Fq poly_input_eval = fq_zero();
  for (size_t i = 0; i <= input.size(); i++) {
    Fq chi = i == 0 ? fq_one() : input[i - 1];
    for (size_t j = 0; j < nv; j++) chi *= ((i >> (nv - j - 1)) & 1) ? ry[1 + j] : fq_one() - ry[1 + j];
    poly_input_eval += chi;
  }
  Fq ev[3];
  evals(ev);
  // expected = (r_A eA + r_B eB + r_C eC) * ((1 - ry0) comm_vars_at_ry + ry0 commit(poly_input_eval, 0))   (:470-480)
  const Fq k = r_A * ev[0] + r_B * ev[1] + r_C * ev[2];
  const MultiCommitGens& pg1 = gens.gens_pc.gens.gens_1;
  CP expected_post2 = Terms().add(P.comm_vars_at_ry, k * (fq_one() - ry[0])).add(gb.at(pg1.G[0]), k * ry[0] * poly_input_eval).eval();
  equality_verify(P.proof_eq_sc_phase2, g1, t, expected_post2, comm_claim_post_phase2);
  *rx_out = rx;
  *ry_out = ry;
}

// ---- sumcheck.rs, product_tree.rs, sparse_mlpoly.rs: the SPARK part of SNARK::verify. No groups here except the three PolyEvalProofs.
Fq eq_evaluate(const FqVec& r, const FqVec& rx) {  // EqPolynomial::evaluate (dense_mlpoly.rs:60-66)
  require(r.size() == rx.size());
  Fq acc = fq_one();
  for (size_t i = 0; i < rx.size(); i++) acc *= r[i] * rx[i] + (fq_one() - r[i]) * (fq_one() - rx[i]);
  return acc;
}
size_t next_pow2(size_t n) { return (size_t)1 << log_2(n); }  // usize::next_power_of_two: 1 for 0 and 1
// SumcheckInstanceProof::verify (sumcheck.rs:27-61): CompressedUniPoly::decompress against the running claim (unipoly.rs:95-108), e(0) + e(1)
Fq sumcheck_verify(const SumcheckInstanceProof& p, Fq e, size_t num_rounds, size_t degree_bound, Transcript& t, FqVec* r_out) {
  require(p.compressed_polys.size() == num_rounds);  // :38
  FqVec r;
  for (size_t i = 0; i < num_rounds; i++) {
    const FqVec& cp = p.compressed_polys[i];
    require(cp.size() == degree_bound && degree_bound >= 1);  // :44: the degree of the decompressed polynomial is the compressed length
    Fq linear = e - cp[0] - cp[0];
    for (size_t k = 1; k < cp.size(); k++) linear -= cp[k];
    FqVec coeffs;
    coeffs.push_back(cp[0]);
    coeffs.push_back(linear);
    coeffs.insert(coeffs.end(), cp.begin() + 1, cp.end());
    Fq at_one = fq_zero();
    for (auto& c : coeffs) at_one += c;
    require(coeffs[0] + at_one == e);  // :47 (true by construction of the linear term, kept as the reference keeps it)
    t.append_message("poly", "UniPoly_begin");  // unipoly.rs:112-120
    for (auto& c : coeffs) t.append_scalar("coeff", c);
    t.append_message("poly", "UniPoly_end");
    Fq r_i = t.challenge_scalar("challenge_nextround");
    r.push_back(r_i);
    Fq power = r_i;  // UniPoly::evaluate (:72-80)
    e = coeffs[0];
    for (size_t k = 1; k < coeffs.size(); k++) { e += power * coeffs[k]; power *= r_i; }
  }
  *r_out = r;
  return e;
}
// ProductCircuitEvalProofBatched::verify (product_tree.rs:385-485). The reference indexes claims_dotp by the caller's claims_dotp_vec and its
// coefficient vector: lengths that would panic there are a 0 here.
void product_batched_verify(const ProductCircuitEvalProofBatched& P, const FqVec& claims_prod_vec, const FqVec& claims_dotp_vec, size_t len,
                            Transcript& t, FqVec* claims_out, FqVec* claims_dotp_out, FqVec* rand_out) {
  const size_t num_layers = log_2(len), np = claims_prod_vec.size();
  require(P.proof.size() == num_layers);  // :395
  FqVec rand, claims_to_verify = claims_prod_vec, claims_to_verify_dotp;
  for (size_t i = 0; i < num_layers; i++) {
    const bool last = i == num_layers - 1;
    if (last) claims_to_verify.insert(claims_to_verify.end(), claims_dotp_vec.begin(), claims_dotp_vec.end());
    FqVec coeff = t.challenge_vector("rand_coeffs_next_layer", claims_to_verify.size());
    Fq claim = dot(claims_to_verify, coeff);
    FqVec rand_prod;
    Fq claim_last = sumcheck_verify(P.proof[i].proof, claim, i, 3, t, &rand_prod);
    const FqVec &cl = P.proof[i].claims_prod_left, &cr = P.proof[i].claims_prod_right;
    require(cl.size() == np && cr.size() == np);  // :417-418
    for (size_t k = 0; k < np; k++) {
      t.append_scalar("claim_prod_left", cl[k]);
      t.append_scalar("claim_prod_right", cr[k]);
    }
    Fq eq = eq_evaluate(rand, rand_prod);  // :425
    Fq claim_expected = fq_zero();
    for (size_t k = 0; k < np; k++) claim_expected += coeff[k] * (cl[k] * cr[k] * eq);
    if (last) {
      const FqVec &dl = P.claims_dotp[0], &dr = P.claims_dotp[1], &dw = P.claims_dotp[2];
      require(dl.size() == claims_dotp_vec.size() && dr.size() == dl.size() && dw.size() == dl.size());  // the index panics of :444-447, 466-473
      for (size_t k = 0; k < dl.size(); k++) {
        t.append_scalar("claim_dotp_left", dl[k]);
        t.append_scalar("claim_dotp_right", dr[k]);
        t.append_scalar("claim_dotp_weight", dw[k]);
        claim_expected += coeff[k + np] * dl[k] * dr[k] * dw[k];
      }
    }
    require(claim_expected == claim_last);  // :451
    Fq r_layer = t.challenge_scalar("challenge_r_layer");
    claims_to_verify.clear();
    for (size_t k = 0; k < np; k++) claims_to_verify.push_back(cl[k] + r_layer * (cr[k] - cl[k]));
    if (last)
      for (size_t k = 0; k < claims_dotp_vec.size() / 2; k++)
        for (int w = 0; w < 3; w++) {
          const FqVec& c = P.claims_dotp[w];
          claims_to_verify_dotp.push_back(c[2 * k] + r_layer * (c[2 * k + 1] - c[2 * k]));
        }
    rand_prod.insert(rand_prod.begin(), r_layer);
    rand = rand_prod;
  }
  *claims_out = claims_to_verify;
  *claims_dotp_out = claims_to_verify_dotp;
  *rand_out = rand;
}
// ProductLayerProof::verify (sparse_mlpoly.rs:1216-1304): -> (claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops)
void product_layer_verify(const ProductLayerProof& L, size_t num_ops, size_t num_cells, const FqVec& eval, Transcript& t, FqVec* claims_mem,
                          FqVec* rand_mem, FqVec* claims_ops, FqVec* claims_dotp, FqVec* rand_ops) {
  t.append_protocol_name("Sparse polynomial product layer proof");
  const size_t num_instances = eval.size();
  auto side = [&](const Fq& init, const FqVec& rd, const FqVec& wr, const Fq& audit, const char* li, const char* lr, const char* lw, const char* la) {
    require(wr.size() == num_instances && rd.size() == num_instances);  // :1238-1239, 1251-1252
    Fq ws = fq_one(), rs = fq_one();
    for (auto& x : wr) ws *= x;
    for (auto& x : rd) rs *= x;
    require(init * ws == rs * audit);  // :1242, 1255
    t.append_scalar(li, init); t.append_scalars(lr, rd); t.append_scalars(lw, wr); t.append_scalar(la, audit);
  };
  side(L.row_init, L.row_read, L.row_write, L.row_audit, "claim_row_eval_init", "claim_row_eval_read", "claim_row_eval_write", "claim_row_eval_audit");
  side(L.col_init, L.col_read, L.col_write, L.col_audit, "claim_col_eval_init", "claim_col_eval_read", "claim_col_eval_write", "claim_col_eval_audit");
  require(L.eval_val[0].size() == num_instances && L.eval_val[1].size() == num_instances);  // :1264-1265
  FqVec claims_dotp_circuit, claims_prod_circuit, claims_mem_dotp;
  for (size_t i = 0; i < num_instances; i++) {
    require(L.eval_val[0][i] + L.eval_val[1][i] == eval[i]);  // :1268
    t.append_scalar("claim_eval_dotp_left", L.eval_val[0][i]);
    t.append_scalar("claim_eval_dotp_right", L.eval_val[1][i]);
    claims_dotp_circuit.push_back(L.eval_val[0][i]);
    claims_dotp_circuit.push_back(L.eval_val[1][i]);
  }
  for (const FqVec* v : {&L.row_read, &L.row_write, &L.col_read, &L.col_write}) claims_prod_circuit.insert(claims_prod_circuit.end(), v->begin(), v->end());
  product_batched_verify(L.proof_ops, claims_prod_circuit, claims_dotp_circuit, num_ops, t, claims_ops, claims_dotp, rand_ops);
  product_batched_verify(L.proof_mem, {L.row_init, L.row_audit, L.col_init, L.col_audit}, {}, num_cells, t, claims_mem, &claims_mem_dotp, rand_mem);
}
// the n-to-1 reduction of DerefsEvalProof::verify_single (:158-170) and HashLayerProof::verify (:943-955, 968-978): `evals`, a power of two
// of them, bound from the last variable up at the challenges; the joint point is (challenges, r)
Fq combine_n_to_one(FqVec evals, Transcript& t, const char* chal_label, const FqVec& r, FqVec* r_joint) {
  FqVec ch = t.challenge_vector(chal_label, log_2(evals.size()));
  for (size_t i = ch.size(); i-- > 0;) {  // DensePolynomial::bound_poly_var_bot (dense_mlpoly.rs:225-233)
    const size_t n = evals.size() / 2;
    for (size_t k = 0; k < n; k++) evals[k] = evals[2 * k] + ch[i] * (evals[2 * k + 1] - evals[2 * k]);
    evals.resize(n);
  }
  require(evals.size() == 1);  // :167, 952, 976
  *r_joint = ch;
  r_joint->insert(r_joint->end(), r.begin(), r.end());
  return evals[0];
}
// PolyEvalProof::verify_plain (dense_mlpoly.rs:391-403): C_Zr = commit(Zr, 0)
void polyeval_verify_plain(sp_ctx* c, const PolyEvalProof& p, const PolyCommitmentGens& gens, const GenBytes& gb, Transcript& t, const FqVec& r, const Fq& Zr,
                           const PolyCommitment& comm, const sp_points* resident = nullptr) {
  const MultiCommitGens& g1 = gens.gens.gens_1;
  CP C_Zr = commit_gens(g1, {g1.G[0]}, {Zr});
  polyeval_verify(c, p, gens, gb, t, r.data(), r.size(), C_Zr, comm, resident);
}
// HashLayerProof::verify_helper (sparse_mlpoly.rs:837-886)
void hash_verify_helper(const FqVec& rand_mem, const Fq& claim_init, const FqVec& claim_read, const FqVec& claim_write, const Fq& claim_audit,
                        const FqVec& eval_ops_val, const FqVec& eval_ops_addr, const FqVec& eval_read_ts, const Fq& eval_audit_ts, const FqVec& r,
                        const Fq& r_hash, const Fq& r_multiset) {
  const Fq r_hash_sqr = r_hash * r_hash;
  auto hash = [&](const Fq& addr, const Fq& val, const Fq& ts) { return ts * r_hash_sqr + val * r_hash + addr - r_multiset; };
  const size_t len = rand_mem.size();
  require(len < 64);
  Fq eval_init_addr = fq_zero();  // IdentityPolynomial::evaluate (dense_mlpoly.rs:110-116)
  for (size_t i = 0; i < len; i++) eval_init_addr += fq_from_u64((uint64_t)1 << (len - i - 1)) * rand_mem[i];
  const Fq eval_init_val = eq_evaluate(r, rand_mem);
  require(hash(eval_init_addr, eval_init_val, fq_zero()) == claim_init);  // :861
  const size_t k = eval_ops_addr.size();  // the reference indexes the other four by it (:864-876)
  require(eval_ops_val.size() >= k && eval_read_ts.size() >= k && claim_read.size() >= k && claim_write.size() >= k);
  for (size_t i = 0; i < k; i++) require(hash(eval_ops_addr[i], eval_ops_val[i], eval_read_ts[i]) == claim_read[i]);               // :867
  for (size_t i = 0; i < k; i++) require(hash(eval_ops_addr[i], eval_ops_val[i], eval_read_ts[i] + fq_one()) == claim_write[i]);  // :875
  require(hash(eval_init_addr, eval_init_val, eval_audit_ts) == claim_audit);  // :883
}
// HashLayerProof::verify (sparse_mlpoly.rs:888-1018) with DerefsEvalProof::verify (:151-201)
void hash_layer_verify(sp_ctx* c, const HashLayerProof& H, const FqVec& rand_mem, const FqVec& rand_ops, const FqVec& claims_mem, const FqVec& claims_ops,
                       const FqVec& claims_dotp, const SparseMatPolyCommitment& comm, const SparseMatPolyCommitmentGens& gens, const GenBytes& gb,
                       const PolyCommitment& comm_derefs, const FqVec& rx, const FqVec& ry, const Fq& r_hash, const Fq& r_multiset, Transcript& t,
                       const ResidentCommitment& res) {
  t.append_protocol_name("Sparse polynomial hash layer proof");
  const FqVec &eval_row_ops_val = H.eval_derefs[0], &eval_col_ops_val = H.eval_derefs[1];
  require(eval_row_ops_val.size() == eval_col_ops_val.size());  // :910
  {
    t.append_protocol_name("Derefs evaluation proof");
    FqVec ev = eval_row_ops_val;
    ev.insert(ev.end(), eval_col_ops_val.begin(), eval_col_ops_val.end());
    ev.resize(next_pow2(ev.size()), fq_zero());
    t.append_scalars("evals_ops_val", ev);
    FqVec r_joint;
    Fq joint = combine_n_to_one(ev, t, "challenge_combine_n_to_one", rand_ops, &r_joint);
    t.append_scalar("joint_claim_eval", joint);
    polyeval_verify_plain(c, H.proof_derefs, gens.gens_derefs, gb, t, r_joint, joint, comm_derefs);
  }
  require(claims_dotp.size() == 3 * eval_row_ops_val.size());  // :922
  require(H.eval_val.size() >= claims_dotp.size() / 3);        // indexed at :930
  for (size_t i = 0; i < claims_dotp.size() / 3; i++)
    require(claims_dotp[3 * i] == eval_row_ops_val[i] && claims_dotp[3 * i + 1] == eval_col_ops_val[i] && claims_dotp[3 * i + 2] == H.eval_val[i]);
  FqVec evals_ops;
  for (const FqVec* v : {&H.row_addr, &H.row_read_ts, &H.col_addr, &H.col_read_ts, &H.eval_val}) evals_ops.insert(evals_ops.end(), v->begin(), v->end());
  evals_ops.resize(next_pow2(evals_ops.size()), fq_zero());
  t.append_scalars("claim_evals_ops", evals_ops);
  FqVec r_joint_ops, r_joint_mem;
  Fq joint_ops = combine_n_to_one(evals_ops, t, "challenge_combine_n_to_one", rand_ops, &r_joint_ops);
  t.append_scalar("joint_claim_eval_ops", joint_ops);
  polyeval_verify_plain(c, H.proof_ops, gens.gens_ops, gb, t, r_joint_ops, joint_ops, comm.comm_comb_ops, res.ops);
  FqVec evals_mem = {H.row_audit_ts, H.col_audit_ts};
  t.append_scalars("claim_evals_mem", evals_mem);
  Fq joint_mem = combine_n_to_one(evals_mem, t, "challenge_combine_two_to_one", rand_mem, &r_joint_mem);
  t.append_scalar("joint_claim_eval_mem", joint_mem);
  polyeval_verify_plain(c, H.proof_mem, gens.gens_mem, gb, t, r_joint_mem, joint_mem, comm.comm_comb_mem, res.mem);
  // claims_mem = (row init, row audit, col init, col audit), claims_ops = (row read, row write, col read, col write) x num_instances (:986-1015)
  require(claims_mem.size() == 4 && claims_ops.size() % 4 == 0);
  const size_t ni = claims_ops.size() / 4;
  auto part = [&](size_t k) { return FqVec(claims_ops.begin() + k * ni, claims_ops.begin() + (k + 1) * ni); };
  hash_verify_helper(rand_mem, claims_mem[0], part(0), part(1), claims_mem[1], eval_row_ops_val, H.row_addr, H.row_read_ts, H.row_audit_ts, rx, r_hash,
                     r_multiset);
  hash_verify_helper(rand_mem, claims_mem[2], part(2), part(3), claims_mem[3], eval_col_ops_val, H.col_addr, H.col_read_ts, H.col_audit_ts, ry, r_hash,
                     r_multiset);
}
// SparseMatPolyEvalProof::verify (sparse_mlpoly.rs:1516-1553) over PolyEvalNetworkProof::verify (:1354-1416)
void sparse_eval_verify(sp_ctx* c, const SparseMatPolyEvalProof& P, const SparseMatPolyCommitment& comm, const FqVec& rx, const FqVec& ry, const FqVec& evals,
                        const SparseMatPolyCommitmentGens& gens, const GenBytes& gb, Transcript& t, const ResidentCommitment& res) {
  t.append_protocol_name("Sparse polynomial evaluation proof");
  FqVec rxe = rx, rye = ry;  // equalize (:1429-1445): the shorter point gets leading zeros
  if (rx.size() < ry.size()) rxe.insert(rxe.begin(), ry.size() - rx.size(), fq_zero());
  if (ry.size() < rx.size()) rye.insert(rye.begin(), rx.size() - ry.size(), fq_zero());
  require(rxe.size() < 64 && ((size_t)1 << rxe.size()) == comm.num_mem_cells);  // :1531
  t.append_message("derefs_commitment", "begin_derefs_commitment");  // DerefsCommitment::append_to_transcript (:204-210 -> dense_mlpoly.rs:292-300)
  t.append_message("comm_poly_row_col_ops_val", "poly_commitment_begin");
  for (auto& pt : P.comm_derefs.C) t.append_point("poly_commitment_share", pt.data());
  t.append_message("comm_poly_row_col_ops_val", "poly_commitment_end");
  t.append_message("derefs_commitment", "end_derefs_commitment");
  FqVec r_mem_check = t.challenge_vector("challenge_r_hash", 2);
  t.append_protocol_name("Sparse polynomial evaluation proof");  // PolyEvalNetworkProof::protocol_name (:1314-1316)
  const size_t num_instances = evals.size(), num_ops = next_pow2(comm.num_ops), num_cells = (size_t)1 << rxe.size();
  FqVec claims_mem, rand_mem, claims_ops, claims_dotp, rand_ops;
  product_layer_verify(P.proof_prod_layer, num_ops, num_cells, evals, t, &claims_mem, &rand_mem, &claims_ops, &claims_dotp, &rand_ops);
  require(claims_mem.size() == 4 && claims_ops.size() == 4 * num_instances && claims_dotp.size() == 3 * num_instances);  // :1379-1381
  hash_layer_verify(c, P.proof_hash_layer, rand_mem, rand_ops, claims_mem, claims_ops, claims_dotp, comm, gens, gb, P.comm_derefs, rxe, rye, r_mem_check[0],
                    r_mem_check[1], t, res);
}

// ---- bincode 1.3 of NIZK { R1CSProof, (Vec<Scalar>, Vec<Scalar>) }: fixed-width little-endian integers, u64 lengths, Scalars as their raw
// Montgomery limbs (ristretto255.rs:198-199). Every length is checked against the bytes that remain before anything is allocated.
struct Rd {
  const uint8_t* p;
  size_t n, o = 0;
  bool ok = true;
  size_t left() const { return n - o; }
  uint64_t u64() {
    if (!ok || left() < 8) { ok = false; return 0; }
    uint64_t x = 0;
    for (int i = 0; i < 8; i++) x |= (uint64_t)p[o + i] << (8 * i);
    o += 8;
    return x;
  }
  size_t len(size_t min_elem_bytes) {  // a Vec length whose elements must still fit into the input
    uint64_t k = u64();
    if (!ok || k > left() / min_elem_bytes) { ok = false; return 0; }
    return (size_t)k;
  }
  Fq fq() {
    Fq x = fq_zero();
    if (!ok || left() < 32) { ok = false; return x; }
    for (int w = 0; w < 4; w++) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[o + 8 * w + i] << (8 * i); x.l[w] = v; }
    o += 32;
    if (!limbs_below_q(x.l)) { ok = false; return fq_zero(); }  // limbs >= q are not a Scalar
    return x;
  }
  CP cp() {
    CP c{};
    if (!ok || left() < 32) { ok = false; return c; }
    memcpy(c.data(), p + o, 32);
    o += 32;
    return c;
  }
  FqVec fqv() { size_t k = len(32); FqVec v(k); for (size_t i = 0; i < k && ok; i++) v[i] = fq(); return v; }
  std::vector<CP> cpv() { size_t k = len(32); std::vector<CP> v(k); for (size_t i = 0; i < k && ok; i++) v[i] = cp(); return v; }
};
void r_dpp(Rd& r, DotProductProof& p) { p.delta = r.cp(); p.beta = r.cp(); p.z = r.fqv(); p.z_delta = r.fq(); p.z_beta = r.fq(); }
void r_zksc(Rd& r, ZKSumcheckInstanceProof& p) {
  p.comm_polys = r.cpv(); p.comm_evals = r.cpv();
  size_t k = r.len(136);  // a DotProductProof is at least 2 points, a length and 2 scalars
  p.proofs.resize(k);
  for (size_t i = 0; i < k && r.ok; i++) r_dpp(r, p.proofs[i]);
}
void r_eq(Rd& r, EqualityProof& p) { p.alpha = r.cp(); p.z = r.fq(); }
void r_r1cs(Rd& r, R1CSProof& p) {  // field order of r1csproof.rs:21-37, as serialize_r1cs_proof writes it
  p.comm_vars.C = r.cpv();
  r_zksc(r, p.sc_proof_phase1);
  for (int i = 0; i < 4; i++) p.claims_phase2[i] = r.cp();
  p.pok_claims_phase2.alpha = r.cp(); p.pok_claims_phase2.z1 = r.fq(); p.pok_claims_phase2.z2 = r.fq();
  p.proof_prod.alpha = r.cp(); p.proof_prod.beta = r.cp(); p.proof_prod.delta = r.cp();
  for (int i = 0; i < 5; i++) p.proof_prod.z[i] = r.fq();
  r_eq(r, p.proof_eq_sc_phase1);
  r_zksc(r, p.sc_proof_phase2);
  p.comm_vars_at_ry = r.cp();
  DotProductProofLog& d = p.proof_eval_vars_at_ry.proof;
  d.bullet.L_vec = r.cpv(); d.bullet.R_vec = r.cpv(); d.delta = r.cp(); d.beta = r.cp(); d.z1 = r.fq(); d.z2 = r.fq();
  r_eq(r, p.proof_eq_sc_phase2);
}
void r_pe(Rd& r, PolyEvalProof& p) {
  DotProductProofLog& d = p.proof;
  d.bullet.L_vec = r.cpv(); d.bullet.R_vec = r.cpv(); d.delta = r.cp(); d.beta = r.cp(); d.z1 = r.fq(); d.z2 = r.fq();
}
void r_batched(Rd& r, ProductCircuitEvalProofBatched& p) {  // product_tree.rs:133-139, 162-166; sumcheck.rs:17-20
  size_t k = r.len(24);  // a LayerProofBatched is at least three lengths
  p.proof.resize(k);
  for (size_t i = 0; i < k && r.ok; i++) {
    LayerProofBatched& l = p.proof[i];
    size_t m = r.len(8);  // a CompressedUniPoly is at least a length
    l.proof.compressed_polys.resize(m);
    for (size_t j = 0; j < m && r.ok; j++) l.proof.compressed_polys[j] = r.fqv();
    l.claims_prod_left = r.fqv(); l.claims_prod_right = r.fqv();
  }
  for (int i = 0; i < 3; i++) p.claims_dotp[i] = r.fqv();
}
void r_evalproof(Rd& r, SparseMatPolyEvalProof& p) {  // sparse_mlpoly.rs:1418-1422, 1307-1311, 1021-1028, 680-689: as w_evalproof writes it
  p.comm_derefs.C = r.cpv();
  ProductLayerProof& L = p.proof_prod_layer;
  L.row_init = r.fq(); L.row_read = r.fqv(); L.row_write = r.fqv(); L.row_audit = r.fq();
  L.col_init = r.fq(); L.col_read = r.fqv(); L.col_write = r.fqv(); L.col_audit = r.fq();
  L.eval_val[0] = r.fqv(); L.eval_val[1] = r.fqv();
  r_batched(r, L.proof_mem); r_batched(r, L.proof_ops);
  HashLayerProof& h = p.proof_hash_layer;
  h.row_addr = r.fqv(); h.row_read_ts = r.fqv(); h.row_audit_ts = r.fq();
  h.col_addr = r.fqv(); h.col_read_ts = r.fqv(); h.col_audit_ts = r.fq();
  h.eval_val = r.fqv(); h.eval_derefs[0] = r.fqv(); h.eval_derefs[1] = r.fqv();
  r_pe(r, h.proof_ops); r_pe(r, h.proof_mem); r_pe(r, h.proof_derefs);
}
}  // namespace

// ---- verifier-only generators: the streams of SNARKGens / NIZKGens as resident point sets. A verification multiplies one range of a stream per
// opening (G_hat) and combines a handful of generators on the host; neither needs the prover's fixed-base window tables, which take most of
// the device and seconds to build. The set comes out of the same uniform bytes through the same one-way map, on the device, with its encodings.
GensStream GensStream::verifier_only(sp_ctx* c, const char* label, size_t npoints) {
  GensStream s;
  s.c = c;
  const std::vector<uint8_t> uniform = uniform_bytes(label, npoints);
  s.compressed.resize(32 * npoints);
  sp_points* p = nullptr;
  int32_t rc = sp_points_from_uniform(c, uniform.data(), npoints, s.compressed.data(), &p);
  if (rc != SP_OK) throw dev_error("sp_points_from_uniform", rc);
  s.pts = std::shared_ptr<sp_points>(p, [](sp_points* q) { sp_points_free(q); });
  return s;
}
NIZKGens NIZKGens::verifier_only(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs) {
  const GensLayout l(num_cons, num_vars, num_inputs, 1);
  NIZKGens g;
  g.stream_sat = GensStream::verifier_only(ctx.h, "gens_r1cs_sat", l.sat_points);
  g.index(l);
  return g;
}
SNARKGens SNARKGens::verifier_only(Ctx& ctx, size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_nz_entries) {
  const GensLayout l(num_cons, num_vars, num_inputs, num_nz_entries);
  SNARKGens g;
  g.stream_sat = GensStream::verifier_only(ctx.h, "gens_r1cs_sat", l.sat_points);
  g.stream_eval = GensStream::verifier_only(ctx.h, "gens_r1cs_eval", l.eval_points);
  g.index(l);
  return g;
}
static size_t stream_resident_bytes(const GensStream& s) { return s.g ? sp_gens_table_bytes(s.g) : sp_points_table_bytes(s.pts.get()); }
size_t NIZKGens::resident_bytes() const { return stream_resident_bytes(stream_sat); }
size_t SNARKGens::resident_bytes() const { return stream_resident_bytes(stream_sat) + stream_resident_bytes(stream_eval); }

// ---- the commitment of a circuit, computed by the verifier: SNARK::encode (lib.rs:325-336) is public preprocessing both parties may run. The
// dense representation is the prover's (encode_dense), multi_commit (sparse_mlpoly.rs:483-503) commits comb_ops and comb_mem without blinds, and
// the tables go when this returns. DensePolynomial::commit's L rows of R scalars (dense_mlpoly.rs:179-204) over gens_n: the window tables of the
// prover's generators (poly_commit), or, under verifier-only ones, gens_n's range of the stream's resident set — sp_commit_rows_points.
ComputationCommitment SNARK::encode_commitment(Ctx& ctx, const Instance& inst, const SNARKGens& gens) {
  MultiSparseMatPolynomialAsDense d;
  encode_dense(ctx, inst, &d);
  auto commit = [&](const DevTable& Z, const PolyCommitmentGens& pg) {
    const size_t num_vars = log_2(Z.len());
    if (!gens.is_verifier_only()) return poly_commit(ctx.h, Z, num_vars, pg, nullptr);
    const size_t Ls = (size_t)1 << (num_vars / 2), Rs = (size_t)1 << (num_vars - num_vars / 2);
    const MultiCommitGens& g = pg.gens.gens_n;
    if (g.n() != Rs || Z.len() != Ls * Rs) throw Error("SNARK::encode_commitment: the generators were made for another instance shape");
    std::vector<uint8_t> out(32 * Ls);
    const int32_t rc = sp_commit_rows_points(ctx.h, g.p, g.G[0], Z.h, 0, Ls, Rs, out.data());
    if (rc != SP_OK) throw dev_error("sp_commit_rows_points", rc);
    PolyCommitment pc;
    pc.C.resize(Ls);
    for (size_t i = 0; i < Ls; i++) memcpy(pc.C[i].data(), &out[32 * i], 32);
    return pc;
  };
  ComputationCommitment comm;
  comm.num_cons = inst.num_cons; comm.num_vars = inst.num_vars; comm.num_inputs = inst.num_inputs;
  comm.comm.batch_size = d.batch_size; comm.comm.num_ops = d.num_ops; comm.comm.num_mem_cells = d.num_mem_cells;
  comm.comm.comm_comb_ops = commit(d.comb_ops, gens.gens_r1cs_eval.gens_ops);
  comm.comm.comm_comb_mem = commit(d.comb_mem, gens.gens_r1cs_eval.gens_mem);
  return comm;
}

bool SNARK::deserialize(const uint8_t* bytes, size_t len, SNARK* out) {
  if (!bytes || !out) return false;
  Rd r{bytes, len};
  r_r1cs(r, out->r1cs_sat_proof);
  for (int i = 0; i < 3; i++) out->inst_evals[i] = r.fq();
  r_evalproof(r, out->r1cs_eval_proof);
  return r.ok && r.o == len;  // trailing bytes are malformed
}

// What encode produces and nothing else (r1cs.rs:33-48 -> sparse_mlpoly.rs:483-503): three matrices; comb_ops holds 15 polynomials of num_ops
// entries padded to 16, comb_mem the two audit_ts of num_mem_cells, and a commitment to 2^v entries has 2^(v/2) shares (dense_mlpoly.rs:86-88).
bool ComputationCommitment::deserialize(const uint8_t* bytes, size_t len, ComputationCommitment* out) {
  if (!bytes || !out) return false;
  Rd r{bytes, len};
  const uint64_t kMax = (uint64_t)1 << 32;
  uint64_t h[6];
  for (int i = 0; i < 6; i++) h[i] = r.u64();
  if (!r.ok) return false;
  out->num_cons = h[0]; out->num_vars = h[1]; out->num_inputs = h[2];
  out->comm.batch_size = h[3]; out->comm.num_ops = h[4]; out->comm.num_mem_cells = h[5];
  if (h[0] < 1 || h[0] > kMax || h[1] < 1 || h[1] > kMax || h[2] > kMax || h[3] != 3 || h[4] < 1 || h[4] > kMax || h[5] < 1 || h[5] > kMax) return false;
  out->comm.comm_comb_ops.C = r.cpv();
  out->comm.comm_comb_mem.C = r.cpv();
  if (!r.ok || r.o != len) return false;
  auto pow2_share_count = [](size_t n) { return n >= 1 && n <= 65536 && (n & (n - 1)) == 0; };
  const size_t n_ops = out->comm.comm_comb_ops.C.size(), n_mem = out->comm.comm_comb_mem.C.size();
  if (!pow2_share_count(n_ops) || !pow2_share_count(n_mem)) return false;
  return n_ops == (size_t)1 << ((log_2(h[4]) + 4) / 2) && n_mem == (size_t)1 << ((log_2(h[5]) + 1) / 2);
}

bool NIZK::deserialize(const uint8_t* bytes, size_t len, NIZK* out) {
  if (!bytes || !out) return false;
  Rd r{bytes, len};
  r_r1cs(r, out->r1cs_sat_proof);
  out->rx = r.fqv();
  out->ry = r.fqv();
  return r.ok && r.o == len;  // trailing bytes are malformed
}

namespace {
// NIZK::verify after the two things that belong to the call and not to the proof (the inputs' count and the instance's digest, which
// NIZK::verify_many takes once for all its proofs). With a gate on the thread the evaluation of the instance is posted there, like C_LZ and G_hat.
int nizk_verify_body(const NIZK& P, Ctx& ctx, const Instance& inst, const FqVec& inputs, Transcript& t, const NIZKGens& gens, const std::vector<uint8_t>& digest) {
  sp_ctx* c = ctx.h;
  const FqVec &rx = P.rx, &ry = P.ry;
  t.append_protocol_name("Spartan NIZK proof");
  t.append_message("R1CSShapeDigest", digest.data(), digest.size());
  // R1CSInstance::evaluate(claimed_rx, claimed_ry) (lib.rs:565 -> r1cs.rs:300-303) is started now and collected when the last check needs it
  if (rx.size() != log_2(inst.num_cons) || ry.size() != log_2(2 * inst.num_vars)) return 0;  // cannot equal the challenges (lib.rs:580-581)
  struct Eval {
    DevTable tx, ty;
    sp_job* job = nullptr;
    ~Eval() { if (job) { uint8_t sink[96]; (void)sp_job_wait(job, sink); } }
  } ev;
  const bool gated = tl_seat.gate != nullptr;
  if (gated) {  // the batch's one job, at this proof's own point: started by the leader, owned by the batch
    DevAns a = tl_seat.gate->post(tl_seat.member, DevKey{DevKey::EVAL_START, &inst, 0, 0, 0}, DevReq{nullptr, U(rx), U(ry)});
    spx(a.rc, "sp_sparse_evaluate_many_begin");
  } else {
    sp_table* h = nullptr;
    spx(sp_eq_expand(c, U(rx), rx.size(), &h), "sp_eq_expand");
    ev.tx = DevTable(c, h);
    spx(sp_eq_expand(c, U(ry), ry.size(), &h), "sp_eq_expand");
    ev.ty = DevTable(c, h);
    const sp_sparse* ms[3] = {inst.dA, inst.dB, inst.dC};
    spx(sp_sparse_evaluate_begin(c, ms, 3, ev.tx.h, ev.ty.h, &ev.job), "sp_sparse_evaluate_begin");
  }
  EvalsFn evals = [&](Fq out[3]) {
    if (gated) {
      DevAns a = tl_seat.gate->post(tl_seat.member, DevKey{DevKey::EVAL_COLLECT, &inst, 0, 0, 0}, DevReq{nullptr, nullptr});
      spx(a.rc, "sp_job_wait");
      for (int k = 0; k < 3; k++) memcpy(out[k].l, a.ev + 4 * k, 32);
      return;
    }
    uint8_t e3[96];
    sp_job* j = ev.job;
    ev.job = nullptr;
    spx(sp_job_wait(j, e3), "sp_job_wait");
    for (int k = 0; k < 3; k++) memcpy(out[k].l, e3 + 32 * k, 32);
  };
  try {
    FqVec vx, vy;
    r1cs_verify(c, P.r1cs_sat_proof, inst.num_vars, inst.num_cons, inputs, evals, t, gens.gens_r1cs_sat, GenBytes{gens.stream_sat.compressed}, &vx, &vy);
    if (vx != rx || vy != ry) return 0;  // lib.rs:580-581
  } catch (const Reject&) {
    return 0;
  }
  return 1;
}
}  // namespace

int NIZK::verify(Ctx& ctx, const Instance& inst, const FqVec& inputs, Transcript& t, const NIZKGens& gens) const {
  if (inputs.size() != inst.num_inputs) throw Error("InvalidNumberOfInputs");  // lib.rs:569: the caller's error, not the proof's
  return nizk_verify_body(*this, ctx, inst, inputs, t, gens, inst.compute_digest());  // lib.rs:559, as NIZK::prove absorbs it
}

int SNARK::verify(Ctx& ctx, const ComputationCommitment& comm, const FqVec& inputs, Transcript& t, const SNARKGens& gens, const ResidentCommitment& res) const {
  sp_ctx* c = ctx.h;
  t.append_protocol_name("Spartan SNARK proof");
  t.append_u64("num_cons", comm.num_cons);  // the commitment as SNARK::prove appends it (r1cs.rs:58-65, sparse_mlpoly.rs:348-361)
  t.append_u64("num_vars", comm.num_vars);
  t.append_u64("num_inputs", comm.num_inputs);
  t.append_u64("batch_size", comm.comm.batch_size);
  t.append_u64("num_ops", comm.comm.num_ops);
  t.append_u64("num_mem_cells", comm.comm.num_mem_cells);
  auto append_shares = [&](const char* label, const PolyCommitment& pc) {  // dense_mlpoly.rs:292-300
    t.append_message(label, "poly_commitment_begin");
    for (auto& pt : pc.C) t.append_point("poly_commitment_share", pt.data());
    t.append_message(label, "poly_commitment_end");
  };
  append_shares("comm_comb_ops", comm.comm.comm_comb_ops);
  append_shares("comm_comb_mem", comm.comm.comm_comb_mem);
  if (!res.ops || !res.mem) throw Error("SNARK::verify: the commitment's resident point sets are missing");
  if (inputs.size() != comm.num_inputs) throw Error("InvalidNumberOfInputs");  // lib.rs:437: the caller's error, not the proof's
  if (comm.num_cons < 1 || comm.num_vars < 1) return 0;
  EvalsFn evals = [&](Fq out[3]) { for (int k = 0; k < 3; k++) out[k] = inst_evals[k]; };  // lib.rs:439-446: the values the proof claims
  try {
    FqVec rx, ry;
    r1cs_verify(c, r1cs_sat_proof, comm.num_vars, comm.num_cons, inputs, evals, t, gens.gens_r1cs_sat, GenBytes{gens.stream_sat.compressed}, &rx, &ry);
    t.append_scalar("Ar_claim", inst_evals[0]);  // lib.rs:450-453
    t.append_scalar("Br_claim", inst_evals[1]);
    t.append_scalar("Cr_claim", inst_evals[2]);
    sparse_eval_verify(c, r1cs_eval_proof, comm.comm, rx, ry, {inst_evals[0], inst_evals[1], inst_evals[2]}, gens.gens_r1cs_eval,
                       GenBytes{gens.stream_eval.compressed}, t, res);  // r1cs.rs:351-366
  } catch (const Reject&) {
    return 0;
  }
  return 1;
}

// ---- SNARK::verify_many: K proofs of one circuit, each verified by SNARK::verify itself on a thread of its own, in lock step through a gate.
namespace {
constexpr size_t kVerifyBatch = 64;              // proofs (threads) in lock step; a longer list is cut into batches of this size

// The batch leader's side of the gate: one device call for a group of requests with equal keys. Runs on one thread at a time, and it is the
// only code of a batch that touches the context. A device failure is thrown: every member of the rendezvous gets it.
void serve_group(sp_ctx* c, const DevKey& key, const std::vector<const DevReq*>& reqs, std::vector<DevAns>& answers) {
  const size_t G = reqs.size(), n = key.n;
  answers.assign(G, DevAns());
  std::vector<uint64_t> S;
  std::vector<uint8_t> pts, out;
  std::vector<int32_t> status;
  // the group in calls of at most `step` members: the whole group unless n K passes the library's cap (n >= 2^14 at 64 proofs)
  size_t step = n && SP_MSM_MANY_MAX_TERMS / n ? SP_MSM_MANY_MAX_TERMS / n : 1;
  if (step > SP_MSM_MANY_MAX_K) step = SP_MSM_MANY_MAX_K;
  if (key.kind == DevKey::ROWS) step = G;
  for (size_t k0 = 0; k0 < G; k0 += step) {
    const size_t k = std::min(step, G - k0);
    S.resize(4 * n * k);
    out.assign(32 * k, 0);
    for (size_t i = 0; i < k; i++) memcpy(S.data() + 4 * n * i, reqs[k0 + i]->S, 32 * n);
    if (key.kind == DevKey::VAR) {
      pts.resize(32 * n * k);
      status.assign(k, SP_OK);
      for (size_t i = 0; i < k; i++) memcpy(pts.data() + 32 * n * i, reqs[k0 + i]->points, 32 * n);
      int32_t rc = sp_msm_var_many(c, pts.data(), S.data(), n, k, out.data(), status.data());
      if (rc != SP_OK) throw dev_error("sp_msm_var_many", rc);
      for (size_t i = 0; i < k; i++) answers[k0 + i].rc = status[i];  // SP_EPOINT: a Reject for that proof alone
    } else if (key.kind == DevKey::POINTS) {
      int32_t rc = sp_msm_points_range_many(c, (const sp_points*)key.obj, key.g_off, n, S.data(), k, out.data());  // a whole set: the range (0, count)
      if (rc != SP_OK) throw dev_error("sp_msm_points_range_many", rc);
    } else {
      int32_t rc = sp_commit_rows(c, (const sp_gens*)key.obj, key.g_off, key.h, S.data(), k, n, nullptr, out.data());
      if (rc != SP_OK) throw dev_error("sp_commit_rows", rc);
    }
    for (size_t i = 0; i < k; i++) memcpy(answers[k0 + i].out.data(), out.data() + 32 * i, 32);
  }
}

// one batch of at most kVerifyBatch parsed proofs, one thread each behind a gate served by `serve`: verdict[m] = verify_one(m)
void run_batch(size_t K, VerifyGate::ServeFn serve, const std::function<int(size_t)>& verify_one, const char* who, int* verdict) {
  VerifyGate gate(K, std::move(serve));
  std::mutex err_mu;
  std::string err;  // the first error of a worker, carried to the caller's thread
  bool have_err = false;
  auto note = [&](const char* what) {
    std::lock_guard<std::mutex> lk(err_mu);
    if (!have_err) { have_err = true; err = what; }
  };
  auto work = [&](size_t m) {
    tl_seat = GateSeat{&gate, m};
    GateMember<VerifyGate> seat(gate, m);  // leaves on return and on exception: a proof rejected early never holds the others up
    try {
      verdict[m] = verify_one(m);
    } catch (const std::exception& e) {
      note(e.what());
    } catch (...) {
      note((std::string(who) + ": unknown exception in a verification").c_str());
    }
    tl_seat = GateSeat();
  };
  std::vector<std::thread> threads;
  size_t started = 0;
  try {
    for (; started < K; started++) threads.emplace_back(work, started);
  } catch (const std::exception& e) {
    note((std::string(who) + ": cannot start a thread: " + e.what()).c_str());
    for (size_t m = started; m < K; m++) gate.leave(m);  // the others must not wait for members that never come
  }
  for (auto& th : threads) th.join();
  if (have_err) throw Error(err);  // on purpose the call's error: verify_many then returns no verdict at all, those of earlier batches of 64 included
}
void verify_batch(Ctx& ctx, const ComputationCommitment& comm, const SNARK* const* proofs, const FqVec* const* inputs, size_t K, const char* label,
                  const SNARKGens& gens, const ResidentCommitment& res, int* verdict) {
  sp_ctx* c = ctx.h;
  run_batch(K, [c](const DevKey& key, const std::vector<size_t>&, const std::vector<const DevReq*>& reqs, std::vector<DevAns>& answers) {
    serve_group(c, key, reqs, answers);
  }, [&](size_t m) {
    Transcript t(label);
    return proofs[m]->verify(ctx, comm, *inputs[m], t, gens, res);
  }, "SNARK::verify_many", verdict);
}

// The evaluation job of a NIZK batch. It belongs to the BATCH: the leader of the first rendezvous starts it for the members that posted a
// point, the leader of the collect rendezvous waits for it once and hands every member its three values. A member that left in between never
// touches it; if nobody collects (every member was rejected on the way), the calling thread waits for it after the join — drain(), by then the
// only thread left. Touched by one leader at a time, like the context.
struct EvalBatch {
  static_assert(kVerifyBatch <= SP_EVAL_MANY_MAX_K, "a batch's evaluation is one call");
  sp_job* job = nullptr;
  size_t count = 0;                // points of the job
  std::vector<size_t> slot;        // member -> its index in the job
  std::vector<uint64_t> vals;      // 12 limbs a point once collected
  bool collected = false;
  explicit EvalBatch(size_t K) : slot(K, (size_t)-1) {}
  ~EvalBatch() { drain(); }
  void drain() noexcept {
    if (!job) return;
    std::vector<uint8_t> sink(96 * count);
    (void)sp_job_wait(job, sink.data());
    job = nullptr;
  }
  void start(sp_ctx* c, const Instance& inst, const std::vector<size_t>& members, const std::vector<const DevReq*>& reqs, std::vector<DevAns>& answers) {
    if (job || collected) throw std::logic_error("NIZK::verify_many: a second evaluation in one batch");
    const size_t G = reqs.size(), ex = log_2(inst.num_cons), ey = log_2(2 * inst.num_vars);
    std::vector<uint64_t> rx(4 * ex * G), ry(4 * ey * G);
    for (size_t i = 0; i < G; i++) {  // every member has checked its lengths before posting
      memcpy(rx.data() + 4 * ex * i, reqs[i]->S, 32 * ex);
      memcpy(ry.data() + 4 * ey * i, reqs[i]->S2, 32 * ey);
      slot[members[i]] = i;
    }
    const sp_sparse* ms[3] = {inst.dA, inst.dB, inst.dC};
    int32_t rc = sp_sparse_evaluate_many_begin(c, ms, 3, rx.data(), ex, ry.data(), ey, G, &job);
    if (rc != SP_OK) { job = nullptr; throw dev_error("sp_sparse_evaluate_many_begin", rc); }
    count = G;
    answers.assign(G, DevAns());
  }
  void collect(const std::vector<size_t>& members, std::vector<DevAns>& answers) {
    if (!collected) {
      if (!job) throw std::logic_error("NIZK::verify_many: an evaluation collected before it was started");
      vals.assign(12 * count, 0);
      sp_job* j = job;
      job = nullptr;  // sp_job_wait frees it, whatever it returns
      int32_t rc = sp_job_wait(j, (uint8_t*)vals.data());
      if (rc != SP_OK) throw dev_error("sp_job_wait", rc);
      collected = true;
    }
    answers.assign(members.size(), DevAns());
    for (size_t i = 0; i < members.size(); i++) {
      const size_t s = slot.at(members[i]);
      if (s >= count) throw std::logic_error("NIZK::verify_many: a member collects an evaluation it did not start");
      memcpy(answers[i].ev, vals.data() + 12 * s, 96);
    }
  }
};
void nizk_verify_batch(Ctx& ctx, const Instance& inst, const NIZK* const* proofs, const FqVec* const* inputs, size_t K, const char* label, const NIZKGens& gens,
                       const std::vector<uint8_t>& digest, int* verdict) {
  sp_ctx* c = ctx.h;
  EvalBatch eval(K);  // outlives the threads: run_batch joins them all before it returns or throws
  run_batch(K, [c, &inst, &eval](const DevKey& key, const std::vector<size_t>& members, const std::vector<const DevReq*>& reqs, std::vector<DevAns>& answers) {
    if (key.kind == DevKey::EVAL_START) eval.start(c, inst, members, reqs, answers);
    else if (key.kind == DevKey::EVAL_COLLECT) eval.collect(members, answers);
    else serve_group(c, key, reqs, answers);
  }, [&](size_t m) {
    Transcript t(label);
    return nizk_verify_body(*proofs[m], ctx, inst, *inputs[m], t, gens, digest);
  }, "NIZK::verify_many", verdict);
}

// The list in batches of at most kVerifyBatch: malformed bytes are a -1 and never enter a gate; run(pp, in, K, v) verifies the K parsed
// proofs of a batch in lock step.
template <class Proof, class Run>
std::vector<int> verify_in_batches(const std::vector<std::pair<const uint8_t*, size_t>>& proofs, const std::vector<const FqVec*>& inputs, Run run) {
  std::vector<int> verdict(proofs.size(), -1);
  for (size_t b0 = 0; b0 < proofs.size(); b0 += kVerifyBatch) {
    const size_t kb = std::min(kVerifyBatch, proofs.size() - b0);
    std::vector<Proof> parsed(kb);
    std::vector<const Proof*> pp;
    std::vector<const FqVec*> in;
    std::vector<size_t> where;
    for (size_t i = 0; i < kb; i++)
      if (Proof::deserialize(proofs[b0 + i].first, proofs[b0 + i].second, &parsed[i])) { pp.push_back(&parsed[i]); in.push_back(inputs[b0 + i]); where.push_back(b0 + i); }
    if (pp.empty()) continue;
    std::vector<int> v(pp.size(), 0);
    run(pp.data(), in.data(), pp.size(), v.data());
    for (size_t i = 0; i < pp.size(); i++) verdict[where[i]] = v[i];
  }
  return verdict;
}
}  // namespace

std::vector<int> SNARK::verify_many(Ctx& ctx, const ComputationCommitment& comm, const std::vector<std::pair<const uint8_t*, size_t>>& proofs,
                                    const std::vector<const FqVec*>& inputs, const char* transcript_label, const SNARKGens& gens,
                                    const ResidentCommitment& res) {
  if (inputs.size() != proofs.size() || !transcript_label) throw Error("SNARK::verify_many: bad arguments");
  if (!res.ops || !res.mem) throw Error("SNARK::verify_many: the commitment's resident point sets are missing");
  for (const FqVec* in : inputs)  // lib.rs:437, before any thread starts: the caller's error, not a proof's
    if (!in || in->size() != comm.num_inputs) throw Error("InvalidNumberOfInputs");
  return verify_in_batches<SNARK>(proofs, inputs, [&](const SNARK* const* pp, const FqVec* const* in, size_t K, int* v) {
    verify_batch(ctx, comm, pp, in, K, transcript_label, gens, res, v);
  });
}

std::vector<int> NIZK::verify_many(Ctx& ctx, const Instance& inst, const std::vector<std::pair<const uint8_t*, size_t>>& proofs,
                                   const std::vector<const FqVec*>& inputs, const char* transcript_label, const NIZKGens& gens) {
  if (inputs.size() != proofs.size() || !transcript_label) throw Error("NIZK::verify_many: bad arguments");
  for (const FqVec* in : inputs)  // lib.rs:569, before any thread starts: the caller's error, not a proof's
    if (!in || in->size() != inst.num_inputs) throw Error("InvalidNumberOfInputs");
  if (proofs.empty()) return {};
  const std::vector<uint8_t> digest = inst.compute_digest();  // lib.rs:559: once per call, every proof's transcript absorbs the same bytes
  return verify_in_batches<NIZK>(proofs, inputs, [&](const NIZK* const* pp, const FqVec* const* in, size_t K, int* v) {
    nizk_verify_batch(ctx, inst, pp, in, K, transcript_label, gens, digest, v);
  });
}

}  // namespace spz
