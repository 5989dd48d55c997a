// spartan_amd host driver — SNARK-only part (included into prover.cc inside namespace spz):
// SNARK::encode (lib.rs:325-336), R1CSEvalProof::prove -> SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1447-1514),
// ProductCircuitEvalProofBatched::prove (product_tree.rs:259-383), prove_cubic_batched (sumcheck.rs:254-424).

// ------------------------------------------------------------------ encode: dense representation (sparse_mlpoly.rs:367-427)

// MultiSparseMatPolynomialAsDense of the instance's three matrices, built on the device: what SNARK::encode commits to and keeps as the
// decommitment, and what SNARK::encode_commitment (verifier.cc) commits to and lets go. No generators are involved.
void encode_dense(Ctx& ctx, const Instance& inst, MultiSparseMatPolynomialAsDense* dense) {
  sp_ctx* c = ctx.h;
  size_t N = 0;
  for (size_t n : inst.nnz) N = std::max(N, next_pow2(n));  // num_nz_entries (:349-351)
  size_t nvx = log_2(inst.num_cons), nvy = log_2(2 * inst.num_vars);
  size_t cells = nvx > nvy ? pow2(nvx) : pow2(nvy);
  MultiSparseMatPolynomialAsDense& d = *dense;
  d.batch_size = 3; d.num_ops = N; d.num_mem_cells = cells;
  // comb_ops = merge(row.ops_addr x3, row.read_ts x3, col.ops_addr x3, col.read_ts x3, val x3) padded to a power of two (:414-419)
  d.comb_ops = tab_alloc(c, next_pow2(15 * N));
  d.comb_mem = tab_alloc(c, 2 * cells);  // row.audit_ts extended by col.audit_ts (:420-421)
  // AddrTimestamps::new (:221-254): the sequential timestamp scan per address runs on the device as a stable sort by
  // address + rank-in-run (sp_addr_timestamps); the host only lays the address lists out
  // (round 4) the address lists and the value vectors come from the entry-order copies sp_sparse keeps on the device (sp_sparse_entry_index,
  // sp_sparse_entry_values): no host pass over the 3 x nnz entries and no pageable uploads — they were 43 of SNARK::encode's 50 ms at 2^20
  sp_sparse* dmats[3] = {inst.dA, inst.dB, inst.dC};
  auto side = [&](bool is_row, AddrTimestamps& at, size_t slot0, size_t mem_off) {
    std::vector<sp_index*> lists;
    size_t ts_off[3];
    for (int k = 0; k < 3; k++) {
      // addresses are < cells by construction: rows < num_cons, columns < 2 num_vars (checked by Instance::new / sp_sparse_upload)
      sp_index* h = nullptr;
      SPX(sp_sparse_entry_index(c, dmats[k], is_row ? 0 : 1, N, &h));
      DevIndex ia(c, h);
      SPX(sp_table_from_index(c, ia.h, d.comb_ops.h, (slot0 + k) * N));
      at.ops_addr.push_back(tab_view(c, d.comb_ops, (slot0 + k) * N, N));
      at.read_ts.push_back(tab_view(c, d.comb_ops, (slot0 + 3 + k) * N, N));
      ts_off[k] = (slot0 + 3 + k) * N;
      lists.push_back(ia.h);
      at.ops_addr_usize.push_back(std::move(ia));
    }
    SPX(sp_addr_timestamps(c, lists.data(), 3, cells, d.comb_ops.h, ts_off, d.comb_mem.h, mem_off));
    at.audit_ts = tab_view(c, d.comb_mem, mem_off, cells);
  };
  REQUIRE(inst.num_cons <= cells && 2 * inst.num_vars <= cells);
  side(true, d.row, 0, 0);
  side(false, d.col, 6, cells);
  for (int k = 0; k < 3; k++) {
    SPX(sp_sparse_entry_values(c, dmats[k], d.comb_ops.h, (12 + k) * N, N));
    d.val.push_back(tab_view(c, d.comb_ops, (12 + k) * N, N));
  }
}

void SNARK::encode(Ctx& ctx, const Instance& inst, const SNARKGens& gens, ComputationCommitment* comm, ComputationDecommitment* decomm) {
  if (gens.is_verifier_only()) throw Error("SNARK::encode: verifier-only generators have no fixed-base tables");
  sp_ctx* c = ctx.h;
  encode_dense(ctx, inst, &decomm->dense);
  const MultiSparseMatPolynomialAsDense& d = decomm->dense;
  // multi_commit (:483-503): comb_ops and comb_mem committed without blinds
  comm->num_cons = inst.num_cons; comm->num_vars = inst.num_vars; comm->num_inputs = inst.num_inputs;
  comm->comm.batch_size = d.batch_size; comm->comm.num_ops = d.num_ops; comm->comm.num_mem_cells = d.num_mem_cells;
  comm->comm.comm_comb_ops = poly_commit(c, d.comb_ops, log_2(d.comb_ops.len()), gens.gens_r1cs_eval.gens_ops, nullptr);
  comm->comm.comm_comb_mem = poly_commit(c, d.comb_mem, log_2(d.comb_mem.len()), gens.gens_r1cs_eval.gens_mem, nullptr);
}

static void append_commitment(Transcript& t, const ComputationCommitment& c) { HSPAN("append_commitment");  // r1cs.rs:58-65, sparse_mlpoly.rs:348-361
  t.append_u64("num_cons", c.num_cons);
  t.append_u64("num_vars", c.num_vars);
  t.append_u64("num_inputs", c.num_inputs);
  t.append_u64("batch_size", c.comm.batch_size);
  t.append_u64("num_ops", c.comm.num_ops);
  t.append_u64("num_mem_cells", c.comm.num_mem_cells);
  append_poly_commitment(t, "comm_comb_ops", c.comm.comm_comb_ops);
  append_poly_commitment(t, "comm_comb_mem", c.comm.comm_comb_mem);
}

// ------------------------------------------------------------------ product circuits (product_tree.rs)
struct ProductCircuit {  // all layers in one device store: layer k (n/2^k elements) at offset 2n - 2n/2^k
  DevTable store;
  size_t n = 0;
  size_t num_layers() const { return log_2(n); }
  size_t layer_off(size_t k) const { return 2 * n - 2 * (n >> k); }
  size_t layer_len(size_t k) const { return n >> k; }
};
// ProductCircuit::evaluate (:58-63) for several circuits in one round trip: the product of the two roots of each
static FqVec product_circuits_evaluate(sp_ctx* c, const std::vector<const ProductCircuit*>& ps) { HSPAN("product_circuits_evaluate");
  std::vector<sp_table*> tabs;
  std::vector<size_t> offs;
  for (auto p : ps) { tabs.push_back(p->store.h); offs.push_back(p->layer_off(p->num_layers() - 1)); }
  FqVec lr(2 * ps.size());
  SPX(sp_table_gather(c, tabs.data(), offs.data(), tabs.size(), 2, U(lr)));
  FqVec out(ps.size());
  for (size_t i = 0; i < ps.size(); i++) out[i] = lr[2 * i] * lr[2 * i + 1];
  return out;
}
struct DotProductCircuit { DevTable left, right, weight; };  // :65-109 (halves of cloned tables)

// Rounds on tables of at most this many entries go to the device TWO at a time (sp_sumcheck_bind2_eval_batched): the device
// returns, with a round's evaluations, the cubic in the next challenge that gives the FOLLOWING round's evaluations, so the
// host derives two challenges per round trip. 0 = one round per launch (option sumcheck.double_round_max_len).
// (A resident-kernel alternative — one kernel that stays on the device and is fed challenges through a host-memory mailbox —
// was measured no faster than a launch per round (DESIGN.md §4); its source is kept as bench/experiments/session_kernel.hip.)
// swept on MI355X at 2^20, round 2: 0 / 512 / 2048 / 8192 / 32768 -> 35.6 / 34.4 / 34.7 / 35.5 / 36.5 ms per proof; round 3, after the two-round kernel's line
// values moved to their own lanes (26.8 -> 13 us per launch): 512 / 1024 / 2048 / 4096 / 8192 -> 27.68 / 28.08 / 27.35 / 27.14 / 27.30 (356 / 356 / 337 / 337 / 322 trips)
static size_t double_round_max_len(const sp_ctx* c) { return (size_t)ctx_opt(c, "sumcheck.double_round_max_len"); }
// E(t; r) for t = 0, 2, 3 from the device's weighted sums (M0, M3, T1, T2) per point (spark.hip, k_cubic_bind2_eval)
static void evals_from_coeffs(const Fq S[12], const Fq& r, Fq ev[3]) {
  static const Fq half = fq_invert(fq_from_u64(2));
  Fq om = fq_one() - r, om2 = om * om, r2 = r * r;
  Fq w0 = om2 * om, w1 = om2 * r, w2 = om * r2, w3 = r2 * r;
  for (int k = 0; k < 3; k++) {
    const Fq &M0 = S[4 * k], &M3 = S[4 * k + 1], &T1 = S[4 * k + 2], &T2 = S[4 * k + 3];
    Fq M1 = (T1 - T2) * half - M3, M2 = (T1 + T2) * half - M0;
    ev[k] = M0 * w0 + M1 * w1 + M2 * w2 + M3 * w3;
  }
}
// The last rounds of prove_cubic_batched (sumcheck.rs:287-419) on tables of m <= 8 entries, on the host: tab = [instance][A, B, C][m].
// Per round: the instances' evaluations at t = 0, 2, 3 combined with coeffs (:290-369) go to `message`, which returns the round's
// challenge (transcript + UniPoly in the prover; a fixed list in the CPU test), then every table is bound at it (:379-393).
// On return tab[(i*3+k)*m_in] holds the final value of table k of instance i (the claims of :395-419).
static void cubic_tail_rounds(FqVec& tab, size_t ni, size_t m, const FqVec& coeffs, const std::function<Fq(const Fq ev[3])>& message) {
  const size_t m_in = m;
  auto at = [&](size_t i, int k, size_t z) -> Fq& { return tab[(i * 3 + k) * m_in + z]; };
  while (m >= 2) {
    size_t h = m / 2;
    Fq evc[3] = {fq_zero(), fq_zero(), fq_zero()};
    for (size_t i = 0; i < ni; i++) {
      Fq e0 = fq_zero(), e2 = fq_zero(), e3 = fq_zero();
      for (size_t z = 0; z < h; z++) {
        const Fq &a0 = at(i, 0, z), &a1 = at(i, 0, h + z), &b0 = at(i, 1, z), &b1 = at(i, 1, h + z), &c0 = at(i, 2, z), &c1 = at(i, 2, h + z);
        Fq a2 = a1 + a1 - a0, b2 = b1 + b1 - b0, c2 = c1 + c1 - c0;   // the line through (0, x0), (1, x1) at 2 and at 3
        Fq a3 = a2 + a1 - a0, b3 = b2 + b1 - b0, c3 = c2 + c1 - c0;
        e0 += a0 * b0 * c0; e2 += a2 * b2 * c2; e3 += a3 * b3 * c3;
      }
      evc[0] += e0 * coeffs[i]; evc[1] += e2 * coeffs[i]; evc[2] += e3 * coeffs[i];
    }
    Fq r = message(evc);
    for (size_t i = 0; i < ni; i++)
      for (int k = 0; k < 3; k++)
        for (size_t z = 0; z < h; z++) at(i, k, z) = at(i, k, z) + r * (at(i, k, h + z) - at(i, k, z));
    m = h;
  }
}
// test hooks (tests/test_host_arith.py): the two pieces of host arithmetic of the batched sum-check, without a device
void cubic_coeffs_probe(const Fq S[12], const Fq& r, Fq ev[3]);
void cubic_tail_probe(FqVec& tab, size_t ni, size_t m, const FqVec& coeffs, const FqVec& challenges, FqVec* evs);
struct BatchedOut { SumcheckInstanceProof proof; FqVec r, prodA, prodB; Fq prodC; FqVec dotA, dotB, dotC; };
void cubic_coeffs_probe(const Fq S[12], const Fq& r, Fq ev[3]) { evals_from_coeffs(S, r, ev); }
void cubic_tail_probe(FqVec& tab, size_t ni, size_t m, const FqVec& coeffs, const FqVec& challenges, FqVec* evs) {
  size_t k = 0;
  cubic_tail_rounds(tab, ni, m, coeffs, [&](const Fq ev[3]) {
    evs->push_back(ev[0]); evs->push_back(ev[1]); evs->push_back(ev[2]);
    return challenges.at(k++);
  });
}
// ---- SURVEY 8e for the batched cubic sum-checks (src/sumcheck.rs:254-424 under src/product_tree.rs:259-383): tables by index residue ----
// The same partition as the ZK sum-checks (prover.cc, ResidueShards): shard g of W holds T_g[k] = T[k W + g] of EVERY table of the batch
// (the A and B halves of each product-circuit layer, the shared eq table, the dot-product circuits' three); a round's pair (i, i + len/2)
// stays on one shard while len/2 is a multiple of W, so each shard runs the ordinary batched round kernels on its sub-tables and a round
// exchanges the 3 partial evaluations per INSTANCE (96 * ni bytes per shard; F_q addition is exact, any order gives the same bytes).
// Only the throughput-sized rounds are worth an exchange: the shards run while the tables are longer than twice the two-rounds-per-trip
// threshold, then pack their sub-tables (one DMA each), the buffers are gathered, and the owner scatters them back into the full tables
// (sp_tables_pack / sp_tables_unpack_residues) — the latency-sized rounds continue unsharded exactly as before.
// Virtual shards (W sub-contexts on one GPU) run it on every sum-check long enough to split; lock-step ranks over the callback / RCCL
// transport from the table length the sharding was configured with (option shard.residue_min_log2, default 2^22: DESIGN.md section 6).
struct CubicShards {
  sp_ctx* owner = nullptr;
  std::vector<sp_ctx*> ctxs;
  bool active = false, remote = false;
  size_t W = 0, me = 0, ni = 0;
  std::vector<sp_table*> full;                 // every table once, in hand-over order (A_i, B_i interleaved, then the distinct C tables)
  std::vector<std::vector<DevTable>> sub;      // [local shard][table of `full`]
  std::vector<std::vector<sp_table*>> hA, hB, hC, hAll;  // per local shard: the batch's pointer lists over the sub-tables
  // tables are handed back when a bind would take them below this length: twice the two-rounds-per-trip threshold (8192 entries by default).
  // Option shard.cubic_min_len (a power of two >= 32; 0 = that default) lowers it so that small test instances run sharded rounds too.
  size_t min_len_ = 8192;
  size_t min_len() const { return min_len_; }
  void read_min_len(const sp_ctx* c) {
    const size_t v = (size_t)ctx_opt(c, "shard.cubic_min_len"), d = 2 * double_round_max_len(c) < 64 ? 64 : 2 * double_round_max_len(c);
    min_len_ = (v >= 32 && !(v & (v - 1))) ? v : d;
  }
  void split(sp_ctx* c, const std::vector<sp_table*>& hs, const std::vector<sp_table*>& A, const std::vector<sp_table*>& B, const std::vector<sp_table*>& C) {
    if (hs.empty() || commit_shard_residue_off(c)) return;
    read_min_len(c);
    const size_t len = sp_table_len(hs[0]);
    ctxs = residue_shard_ctxs(c);
    int rank = 0, world = 0, min_log2 = 64;
    if (ctxs.size() >= 2) {
      W = ctxs.size();
    } else if (commit_shard_transport(c, &rank, &world, &min_log2) && min_log2 < 64 && len >= ((size_t)1 << min_log2)) {
      W = (size_t)world; me = (size_t)rank; remote = true;
      ctxs.assign(1, c);
    } else {
      return;
    }
    // worth it only while a few throughput-sized rounds remain: the sub-tables must still be >= 4 entries when the hand-over length is reached
    if (W < 2 || (W & (W - 1)) || len < 4 * min_len() || min_len() / W < 4) { remote = false; return; }
    owner = c; ni = A.size(); full = hs;
    SPX(sp_ctx_sync(c));  // the tables as produced by everything queued on the owning context
    const size_t nloc = remote ? 1 : W;
    sub.resize(nloc); hA.resize(nloc); hB.resize(nloc); hC.resize(nloc); hAll.resize(nloc);
    for (size_t g = 0; g < nloc; g++) {
      std::map<sp_table*, sp_table*> m;
      for (sp_table* t : hs) {
        sp_table* o = nullptr;
        SPX(sp_table_residue_split(ctxs[g], t, W, remote ? me : g, &o));
        sub[g].emplace_back(ctxs[g], o);
        hAll[g].push_back(o);
        m[t] = o;
      }
      for (size_t i = 0; i < ni; i++) { hA[g].push_back(m.at(A[i])); hB[g].push_back(m.at(B[i])); hC[g].push_back(m.at(C[i])); }
    }
    active = true;
  }
  size_t sub_len() const { return sp_table_len(hAll[0][0]); }
  // true while the NEXT bind still leaves tables longer than the hand-over length
  bool keep_going() const { return active && sub_len() * W / 2 >= min_len(); }
  void add_partials(FqVec& ev, std::vector<FqVec>& parts) {
    if (remote) {
      FqVec all(W * 3 * ni);
      memcpy(&all[me * 3 * ni], parts[0].data(), 32 * 3 * ni);
      commit_shard_gather(owner, (uint8_t*)all.data(), 32 * 3 * ni);
      parts.assign(W, FqVec(3 * ni));
      for (size_t g = 0; g < W; g++) memcpy(parts[g].data(), &all[g * 3 * ni], 32 * 3 * ni);
    }
    for (size_t k = 0; k < 3 * ni; k++) {
      Fq acc = fq_zero();
      for (auto& p : parts) acc += p[k];
      ev[k] = acc;
    }
    if (!remote) commit_shard_note_gather(owner, 32 * 3 * ni * parts.size());
  }
  void eval(FqVec& ev) {
    std::vector<FqVec> parts(ctxs.size(), FqVec(3 * ni));
    for (size_t g = 0; g < ctxs.size(); g++) SPX(sp_sumcheck_eval_batched(ctxs[g], hA[g].data(), hB[g].data(), hC[g].data(), ni, U(parts[g])));
    add_partials(ev, parts);
  }
  void bind_eval(const Fq& r, FqVec& ev) {
    std::vector<FqVec> parts(ctxs.size(), FqVec(3 * ni));
    for (size_t g = 0; g < ctxs.size(); g++) SPX(sp_sumcheck_bind_eval_batched(ctxs[g], hA[g].data(), hB[g].data(), hC[g].data(), ni, U(r), U(parts[g])));
    add_partials(ev, parts);
  }
  // the sub-tables go back into the owner's full tables (current length sub_len * W) and the shards are released
  void hand_back() {
    const size_t sl = sub_len(), nt = full.size();
    FqVec all(W * nt * sl);
    if (remote) {
      SPX(sp_tables_pack(owner, hAll[0].data(), nt, sl, all[me * nt * sl].l));
      commit_shard_gather(owner, (uint8_t*)all.data(), 32 * nt * sl);
    } else {
      for (size_t g = 0; g < W; g++) SPX(sp_tables_pack(ctxs[g], hAll[g].data(), nt, sl, all[g * nt * sl].l));
      commit_shard_note_gather(owner, 32 * nt * sl * W);
    }
    SPX(sp_tables_unpack_residues(owner, full.data(), nt, W, sl, U(all)));
    sub.clear(); hA.clear(); hB.clear(); hC.clear(); hAll.clear();
    active = false;
  }
};

// ---- the eq table as a factor (spartan_hip.h, sp_sumcheck_eval_batched_eq): host side of the throughput-sized rounds of a batch whose
// product-circuit instances share C = EqPolynomial::new(rho).evals(). With the tables bound at r_0..r_{j-1}, round j's evaluations are
//     E(t) = kappa_j(t) Q(t) + D(t),   Q(t) = sum_i coeff_i q_i(t) (quadratic),   D(t) = the generic instances' (cubic),
//     kappa_j(t) = K_j eq(t, rho_j) / (1 - rho_j),   K_j = prod_{k<j} eq(r_k, rho_k) / (1 - rho_k),   eq(t, rho) = (1-t)(1-rho) + t rho.
// The device returns q_i(0), q_i(2) and D's four values; Q(1) = (claim - E(0) - D(1)) / kappa_j(1) and Q(3) = Q(0) - 3 Q(1) + 3 Q(2).
// Exact identities in F_q: E(0), E(2), E(3) are the values the generic kernels sum up, so the round polynomial and the proof bytes are
// unchanged. K_j C_original[0..len) IS the bound eq table: multiplying it out (sp_table_scale_prefix) hands over to the generic rounds.
struct EqFactor {
  bool on = false;
  FqVec rho, inv1m, inv_rho;  // the point, 1 / (1 - rho_k), 1 / rho_k
  Fq K = fq_one(), Kinv = fq_one();
  bool enabled = true;  // option spark.eq_factor (A/B switch), set by the caller before begin()
  static constexpr size_t MIN_LEN = 65536;  // the factored kernels are the throughput forms only
  // usable for tables of `len` entries = 2^rho.size() when no coordinate is 0 or 1 (then 1 / (1 - rho) or 1 / rho does not exist)
  bool begin(const FqVec* point, size_t num_rounds, size_t len, size_t np, size_t ni) {
    on = false;
    if (!enabled || !point || point->size() != num_rounds || np == 0 || ni > 24 || len < MIN_LEN) return false;
    rho = *point;
    FqVec d(2 * rho.size());
    for (size_t k = 0; k < rho.size(); k++) { d[2 * k] = fq_one() - rho[k]; d[2 * k + 1] = rho[k]; }
    for (auto& x : d) if (fq_is_zero(x)) return false;
    FqVec pre(d.size());  // Montgomery's trick: one inversion for all of them
    Fq run = fq_one();
    for (size_t k = 0; k < d.size(); k++) { pre[k] = run; run = run * d[k]; }
    Fq inv = fq_invert_vartime(run);  // public values (transcript challenges)
    inv1m.resize(rho.size()); inv_rho.resize(rho.size());
    for (size_t k = d.size(); k-- > 0;) {
      Fq x = inv * pre[k];
      inv = inv * d[k];
      if (k & 1) inv_rho[k / 2] = x; else inv1m[k / 2] = x;
    }
    K = Kinv = fq_one();
    on = true;
    return true;
  }
  // round j's combined evaluations E(0), E(2), E(3) from the device's 4 scalars per instance, the coefficients and the round's claim e
  void combine(size_t j, const FqVec& ev4, const FqVec& coeffs, size_t np, size_t ni, const Fq& e, Fq evc[3]) const {
    Fq Q0 = fq_zero(), Q2 = fq_zero(), D[4] = {fq_zero(), fq_zero(), fq_zero(), fq_zero()};
    for (size_t i = 0; i < np; i++) { Q0 += ev4[4 * i] * coeffs[i]; Q2 += ev4[4 * i + 1] * coeffs[i]; }
    for (size_t i = np; i < ni; i++)
      for (int k = 0; k < 4; k++) D[k] += ev4[4 * i + k] * coeffs[i];
    if (fq_is_zero(K)) { evc[0] = D[0]; evc[1] = D[2]; evc[2] = D[3]; return; }  // a challenge hit a root of eq(., rho_k): the eq table is zero from there on
    const Fq& r = rho[j];
    const Fq three = fq_from_u64(3), five = fq_from_u64(5), two = fq_from_u64(2);
    Fq k0 = K, ks = K * inv1m[j];
    Fq k2 = ks * (three * r - fq_one()), k3 = ks * (five * r - two);
    Fq E0 = k0 * Q0 + D[0];
    Fq E1 = e - E0;
    Fq Q1 = (E1 - D[1]) * Kinv * inv_rho[j] * (fq_one() - r);  // / kappa(1), kappa(1) = K rho / (1 - rho)
    Fq Q3 = Q0 - three * Q1 + three * Q2;
    evc[0] = E0;
    evc[1] = k2 * Q2 + D[2];
    evc[2] = k3 * Q3 + D[3];
  }
  // the tables have been bound at r (round j's challenge)
  void bound(size_t j, const Fq& r) {
    Fq f = (fq_one() - r) * (fq_one() - rho[j]) + r * rho[j];  // eq(r, rho_j)
    K = K * f * inv1m[j];
    Kinv = fq_is_zero(f) ? fq_zero() : Kinv * fq_invert_vartime(f) * (fq_one() - rho[j]);
  }
};

// test hook (tests/test_host_arith.py): the host arithmetic of the factored rounds without a device. ev4: per round, 4 scalars per instance as the
// device returns them; claims: the claim each round starts from; out: E(0), E(2), E(3) per round and the hand-over scalar K after each bind
bool eq_factor_probe(const FqVec& rho, size_t np, size_t ni, const FqVec& coeffs, const FqVec& claims, const FqVec& ev4, const FqVec& challenges, FqVec* evc_out,
                     FqVec* K_out) {
  EqFactor f;
  if (!f.begin(&rho, rho.size(), EqFactor::MIN_LEN, np, ni)) return false;
  const size_t nr = claims.size();
  for (size_t j = 0; j < nr; j++) {
    Fq evc[3];
    FqVec e(ev4.begin() + 4 * ni * j, ev4.begin() + 4 * ni * (j + 1));
    f.combine(j, e, coeffs, np, ni, claims[j], evc);
    evc_out->push_back(evc[0]); evc_out->push_back(evc[1]); evc_out->push_back(evc[2]);
    f.bound(j, challenges[j]);
    K_out->push_back(f.K);
  }
  return true;
}

// SumcheckInstanceProof::prove_cubic_batched (sumcheck.rs:254-424), two rounds per trip on short tables. (A three-rounds-per-trip grid
// form was built and measured in round 3 — 329 instead of 356 trips, +0.3 ms per proof — and is kept as bench/experiments/cubic_grid*.)
// eq_point: when Cpar is EqPolynomial::new(eq_point).evals() (product_tree.rs:279), its throughput-sized rounds run in the factored form
// (EqFactor below)
static BatchedOut prove_cubic_batched(sp_ctx* c, const Fq& claim, size_t num_rounds, std::vector<sp_table*>& Apar, std::vector<sp_table*>& Bpar,
                                      sp_table* Cpar, std::vector<sp_table*>& Aseq, std::vector<sp_table*>& Bseq, std::vector<sp_table*>& Cseq,
                                      const FqVec& coeffs, Transcript& t, const FqVec* eq_point = nullptr) { HSPAN("prove_cubic_batched");
  BatchedOut o;
  Fq e = claim;
  size_t np = Apar.size(), ns = Aseq.size(), ni = np + ns;
  std::vector<sp_table*> A, B, C, distinctC;
  for (size_t k = 0; k < np; k++) { A.push_back(Apar[k]); B.push_back(Bpar[k]); C.push_back(Cpar); }
  for (size_t k = 0; k < ns; k++) { A.push_back(Aseq[k]); B.push_back(Bseq[k]); C.push_back(Cseq[k]); }
  distinctC.push_back(Cpar);
  for (size_t k = 0; k < ns; k++) distinctC.push_back(Cseq[k]);
  FqVec ev(3 * ni);  // per-instance evaluations (one round per launch)
  FqVec ev4(4 * ni);  // the same in the factored form: {q(0), q(2), -, -} or {e(0), e(1), e(2), e(3)} per instance
  EqFactor eqf;
  Fq evc[3], S[12];  // the round's evaluations combined with `coeffs` (:359-369), and the cubic that gives the next round's
  std::vector<sp_table*> hs;  // every table once: A_i, B_i interleaved, then the distinct C tables
  for (size_t i = 0; i < ni; i++) { hs.push_back(A[i]); hs.push_back(B[i]); }
  for (auto x : distinctC) hs.push_back(x);
  FqVec hv(hs.size());
  bool have_heads = false, have_S = false;
  eqf.enabled = ctx_opt(c, "spark.eq_factor") != 0;
  const size_t dmax = double_round_max_len(c);
  auto combine = [&]() {  // :359-369: the instances' evaluations combined with the coefficients
    evc[0] = evc[1] = evc[2] = fq_zero();
    for (size_t i = 0; i < ni; i++) { evc[0] += ev[3 * i] * coeffs[i]; evc[1] += ev[3 * i + 1] * coeffs[i]; evc[2] += ev[3 * i + 2] * coeffs[i]; }
  };
  auto round_message = [&]() {  // :370-381 and :395-396: the round's cubic, its transcript message, the challenge
    UniPoly poly = UniPoly::from_evals({evc[0], e - evc[0], evc[1], evc[2]});
    poly.append_to_transcript(t, "poly");
    Fq r_j = t.challenge_scalar("challenge_nextround");
    o.r.push_back(r_j);
    e = poly.evaluate(r_j);
    o.proof.compressed_polys.push_back(poly.compress());
    return r_j;
  };
  // The last rounds, on this core: once the tables have at most 8 entries the device hands them over with the sums of the
  // trip that produced them (sp_sumcheck_bind2_eval_tables_batched), and the remaining <= 3 rounds — evaluations at t = 0, 2, 3
  // (:290-357), binds (:379-393), final claims (:395-419) — are ~20 us of field arithmetic here instead of two more trips.
  FqVec tail(3 * 8 * ni);
  const bool tail_ok = ctx_opt(c, "sumcheck.host_tail") != 0;
  auto finish_on_host = [&](size_t m, size_t& j) {  // tail = [instance][A, B, C][m]
    cubic_tail_rounds(tail, ni, m, coeffs, [&](const Fq ev[3]) {
      evc[0] = ev[0]; evc[1] = ev[1]; evc[2] = ev[2];
      j += 1;
      return round_message();
    });
    for (size_t i = 0; i < ni; i++) { hv[2 * i] = tail[(i * 3 + 0) * m]; hv[2 * i + 1] = tail[(i * 3 + 1) * m]; }
    hv[2 * ni] = tail[2 * m];  // poly_C_par is instance 0's C (np >= 1 on this path); then the dot-product circuits' own C tables
    for (size_t k = 0; k < ns; k++) hv[2 * ni + 1 + k] = tail[((np + k) * 3 + 2) * m];
    have_heads = true;
  };
  auto tail_given = [&]() { return tail[0].l[0] != ~0ULL || tail[0].l[1] != 0 || tail[0].l[2] != 0 || tail[0].l[3] != 0; };
  size_t j = 0;
  CubicShards cs;  // SURVEY 8e: the throughput-sized rounds on W residue classes of every table (virtual shards, or lock-step ranks from the configured table length)
  if (num_rounds > 0) cs.split(c, hs, A, B, C);
  if (cs.active) {
    cs.eval(ev);
    combine();
    while (cs.active) {
      Fq r_j = round_message();
      j += 1;
      if (cs.keep_going()) {
        cs.bind_eval(r_j, ev);
        combine();
      } else {
        // the last sharded bind (its evaluations are the next round's, like every other's); then the tables return to the owner and the
        // latency-sized rounds continue there in the form their length selects
        cs.bind_eval(r_j, ev);
        combine();
        cs.hand_back();
      }
    }
  } else if (num_rounds > 0) {
    size_t len0 = sp_table_len(A[0]);
    if (tail_ok && np >= 1 && len0 >= 2 && len0 <= 8 && ni <= 21) {
      tail[0] = Fq{{~0ULL, 0, 0, 0}};
      SPX(sp_sumcheck_bind2_eval_tables_batched(c, A.data(), B.data(), C.data(), ni, nullptr, nullptr, U(coeffs), evc[0].l, len0 >= 4 ? S[0].l : nullptr, nullptr, U(tail)));
      REQUIRE(tail_given());
      finish_on_host(len0, j);
    } else if (len0 >= 4 && len0 <= dmax) {
      SPX(sp_sumcheck_eval_coeffs_batched(c, A.data(), B.data(), C.data(), ni, U(coeffs), evc[0].l, S[0].l));
      have_S = true;
    } else if (eqf.begin(eq_point, num_rounds, len0, np, ni)) {
      SPX(sp_sumcheck_eval_batched_eq(c, A.data(), B.data(), C.data(), ni, np, U(ev4)));
      eqf.combine(0, ev4, coeffs, np, ni, e, evc);
    } else {
      SPX(sp_sumcheck_eval_batched(c, A.data(), B.data(), C.data(), ni, U(ev)));
      combine();
    }
  }
  while (j < num_rounds) {
    size_t len = sp_table_len(A[0]);
    Fq r_j = round_message();
    if (eqf.on && len >= EqFactor::MIN_LEN) {
      // a throughput-sized round in the factored form: A and B are bound at r_j, the eq table is only read (its leading len / 4 entries)
      SPX(sp_sumcheck_bind_eval_batched_eq(c, A.data(), B.data(), C.data(), ni, np, U(r_j), U(ev4)));
      eqf.bound(j, r_j);
      j += 1;
      eqf.combine(j, ev4, coeffs, np, ni, e, evc);
      continue;
    }
    if (eqf.on) {
      // hand-over: K * C_original[0 .. len) is the eq table bound at r_0 .. r_{j-1}, which the generic rounds (latency forms) continue with
      SPX(sp_table_scale_prefix(c, Cpar, len, U(eqf.K)));
      eqf.on = false;
    }
    if (have_S && len >= 4) {
      // two rounds in one trip: the next round's evaluations are the device's cubic at r_j, so its message and challenge
      // follow at once; the device then binds at both challenges (:379-393, twice) and evaluates the round after
      evals_from_coeffs(S, r_j, evc);
      Fq r_j1 = round_message();
      size_t n2 = len / 4;
      bool want_tail = tail_ok && np >= 1 && n2 >= 2 && n2 <= 8 && ni <= 21;
      if (want_tail) {
        tail[0] = Fq{{~0ULL, 0, 0, 0}};
        SPX(sp_sumcheck_bind2_eval_tables_batched(c, A.data(), B.data(), C.data(), ni, U(r_j), U(r_j1), U(coeffs), evc[0].l, n2 >= 4 ? S[0].l : nullptr, nullptr, U(tail)));
      } else {
        SPX(sp_sumcheck_bind2_eval_batched(c, A.data(), B.data(), C.data(), ni, U(r_j), U(r_j1), U(coeffs), n2 >= 2 ? evc[0].l : nullptr, n2 >= 4 ? S[0].l : nullptr,
                                           n2 == 1 ? U(hv) : nullptr));
      }
      have_S = n2 >= 4;
      have_heads = n2 == 1;
      j += 2;
      if (want_tail && tail_given()) finish_on_host(n2, j);
      continue;
    }
    // one round per launch: bind everything at r_j (:379-393), fused with the next round's evaluation while length allows; the
    // last bind (length 2 -> 1) also returns the final claims (:395-419) in the same launch
    if (len >= 8 && len / 2 <= dmax) {  // the tables become short with this bind: it also returns the cubic, then two rounds per trip
      size_t n2 = len / 2;
      bool want_tail = tail_ok && np >= 1 && n2 <= 8 && ni <= 21;
      if (want_tail) {
        tail[0] = Fq{{~0ULL, 0, 0, 0}};
        SPX(sp_sumcheck_bind2_eval_tables_batched(c, A.data(), B.data(), C.data(), ni, U(r_j), nullptr, U(coeffs), evc[0].l, S[0].l, nullptr, U(tail)));
      } else {
        SPX(sp_sumcheck_bind2_eval_batched(c, A.data(), B.data(), C.data(), ni, U(r_j), nullptr, U(coeffs), evc[0].l, S[0].l, nullptr));
      }
      have_S = true;
      j += 1;
      if (want_tail && tail_given()) finish_on_host(n2, j);
      continue;
    } else if (len >= 4) {
      SPX(sp_sumcheck_bind_eval_batched(c, A.data(), B.data(), C.data(), ni, U(r_j), U(ev)));
      combine();
    } else {
      SPX(sp_table_bind_top_heads(c, hs.data(), hs.size(), U(r_j), U(hv)));
      have_heads = true;
    }
    j += 1;
  }
  if (!have_heads) SPX(sp_table_heads(c, hs.data(), hs.size(), U(hv)));  // zero rounds: the tables already have length 1
  for (size_t k = 0; k < np; k++) { o.prodA.push_back(hv[2 * k]); o.prodB.push_back(hv[2 * k + 1]); }
  for (size_t k = 0; k < ns; k++) { o.dotA.push_back(hv[2 * (np + k)]); o.dotB.push_back(hv[2 * (np + k) + 1]); o.dotC.push_back(hv[2 * ni + 1 + k]); }
  o.prodC = hv[2 * ni];
  return o;
}

// ProductCircuitEvalProofBatched::prove (product_tree.rs:259-383)
// dotp_evals: DotProductCircuit::evaluate of each dot-product circuit, if the caller already has them (ProductLayerProof::prove
// computes exactly these as its claim_eval_dotp_left/right before it calls this)
// roots: ProductCircuit::evaluate of each circuit, if the caller already has them (ProductLayerProof::prove has just computed and absorbed exactly
// these as its claims: a device trip less per batch)
static ProductCircuitEvalProofBatched product_batched_prove(sp_ctx* c, std::vector<ProductCircuit*>& prods, std::vector<DotProductCircuit*>& dotps,
                                                            Transcript& t, FqVec* rand_out, const FqVec* dotp_evals = nullptr, const FqVec* roots = nullptr) { HSPAN("product_batched_prove");
  REQUIRE(!prods.empty());
  ProductCircuitEvalProofBatched out;
  size_t num_layers = prods[0]->num_layers();
  FqVec claims_to_verify;
  if (roots) {
    REQUIRE(roots->size() == prods.size());
    claims_to_verify = *roots;
  } else {
    std::vector<const ProductCircuit*> ps(prods.begin(), prods.end());
    claims_to_verify = product_circuits_evaluate(c, ps);
  }
  FqVec rand;
  for (size_t li = num_layers; li-- > 0;) {
    size_t len = prods[0]->layer_len(li);
    DevTable poly_C_par = rand.empty() ? tab_upload(c, FqVec{fq_one()}) : tab_eq(c, rand);  // EqPolynomial::new(rand).evals() (:279)
    REQUIRE(poly_C_par.len() == len / 2);
    size_t num_rounds_prod = log_2(len / 2);
    std::vector<DevTable> views;
    std::vector<sp_table*> Apar, Bpar, Aseq, Bseq, Cseq;
    for (auto p : prods) {
      views.push_back(tab_view(c, p->store, p->layer_off(li), len / 2));
      Apar.push_back(views.back().h);
      views.push_back(tab_view(c, p->store, p->layer_off(li) + len / 2, len / 2));
      Bpar.push_back(views.back().h);
    }
    if (li == 0 && !dotps.empty()) {
      REQUIRE(!dotp_evals || dotp_evals->size() == dotps.size());
      for (size_t k = 0; k < dotps.size(); k++) {
        DotProductCircuit* d = dotps[k];
        Fq ev;
        if (dotp_evals) ev = (*dotp_evals)[k];
        else SPX(sp_dot3(c, d->left.h, d->right.h, d->weight.h, 0, d->left.len(), ev.l));  // DotProductCircuit::evaluate (:84-88)
        claims_to_verify.push_back(ev);
        REQUIRE(len / 2 == d->left.len());
      }
      for (auto d : dotps) { Aseq.push_back(d->left.h); Bseq.push_back(d->right.h); Cseq.push_back(d->weight.h); }
    }
    FqVec coeff = t.challenge_vector("rand_coeffs_next_layer", claims_to_verify.size());
    Fq claim = fq_zero();
    for (size_t i = 0; i < claims_to_verify.size(); i++) claim += claims_to_verify[i] * coeff[i];
    BatchedOut bo = prove_cubic_batched(c, claim, num_rounds_prod, Apar, Bpar, poly_C_par.h, Aseq, Bseq, Cseq, coeff, t, rand.empty() ? nullptr : &rand);
    for (size_t i = 0; i < prods.size(); i++) {
      t.append_scalar("claim_prod_left", bo.prodA[i]);
      t.append_scalar("claim_prod_right", bo.prodB[i]);
    }
    if (li == 0 && !dotps.empty()) {
      for (size_t i = 0; i < dotps.size(); i++) {
        t.append_scalar("claim_dotp_left", bo.dotA[i]);
        t.append_scalar("claim_dotp_right", bo.dotB[i]);
        t.append_scalar("claim_dotp_weight", bo.dotC[i]);
      }
      out.claims_dotp[0] = bo.dotA; out.claims_dotp[1] = bo.dotB; out.claims_dotp[2] = bo.dotC;
    }
    Fq r_layer = t.challenge_scalar("challenge_r_layer");
    claims_to_verify.clear();
    for (size_t i = 0; i < prods.size(); i++) claims_to_verify.push_back(bo.prodA[i] + r_layer * (bo.prodB[i] - bo.prodA[i]));
    FqVec ext = {r_layer};
    ext.insert(ext.end(), bo.r.begin(), bo.r.end());
    rand = ext;
    out.proof.push_back(LayerProofBatched{bo.proof, bo.prodA, bo.prodB});
  }
  *rand_out = rand;
  return out;
}

// ------------------------------------------------------------------ layers (sparse_mlpoly.rs:529-678)
struct Derefs { std::vector<DevTable> row_ops_val, col_ops_val; DevTable comb; };
struct ProductLayer { ProductCircuit init; std::vector<ProductCircuit> read_vec, write_vec; ProductCircuit audit; };

// build_hash_layer (:529-604) into the leaves of a circuit store; the multiplication layers are built afterwards for all
// circuits of one size together (sp_product_tree_many)
static ProductCircuit make_circuit_leaves(sp_ctx* c, const sp_table* addr, const sp_table* val, const sp_table* ts, int ts_inc, size_t n, const Fq& r_hash,
                                          const Fq& r_multiset) {
  ProductCircuit p;
  p.n = n;
  p.store = tab_alloc_uninit(c, 2 * n);  // leaves [0, n) and layers [n, 2n - 2) are all written before they are read
  SPX(sp_hash_layer(c, addr, val, ts, ts_inc, n, U(r_hash), U(r_multiset), p.store.h, 0));
  return p;
}
static ProductLayer layers_new(sp_ctx* c, const DevTable& eval_table, const AddrTimestamps& at, const std::vector<DevTable>& ops_val, const Fq& r_hash,
                               const Fq& r_multiset) { HSPAN("layers_new");  // Layers::new (:606-655)
  ProductLayer L;
  size_t cells = eval_table.len();
  size_t n_ops = at.ops_addr.empty() ? 0 : at.ops_addr[0].len();
  for (size_t k = 0; k < at.ops_addr.size(); k++) REQUIRE(at.ops_addr[k].len() == n_ops);
  // round 4: the hash layer writes the first multiplication layer too, and the read and write sets of a matrix (ts and ts + 1: one r_hash^2
  // apart per leaf) come out of one pass over addr, val, ts (sp_hash_layer_first): 1.1 -> 0.8 ms of streaming in front of the first
  // product_circuits_evaluate of a 2^20 proof. Option spark.hash_fuse = 0: the separate launches (A/B switch)
  const bool fuse_env = ctx_opt(c, "spark.hash_fuse") != 0;
  const bool fuse = fuse_env && cells >= 4 && (n_ops == 0 || n_ops >= 4);
  auto blank = [&](size_t n) { ProductCircuit p; p.n = n; p.store = tab_alloc_uninit(c, 2 * n); return p; };
  if (fuse) {
    L.init = blank(cells);
    SPX(sp_hash_layer_first(c, nullptr, eval_table.h, nullptr, 0, cells, U(r_hash), U(r_multiset), L.init.store.h, nullptr));
    for (size_t k = 0; k < at.ops_addr.size(); k++) {
      L.read_vec.push_back(blank(n_ops));
      L.write_vec.push_back(blank(n_ops));
      SPX(sp_hash_layer_first(c, at.ops_addr[k].h, ops_val[k].h, at.read_ts[k].h, 0, n_ops, U(r_hash), U(r_multiset), L.read_vec.back().store.h, L.write_vec.back().store.h));
    }
    L.audit = blank(cells);
    SPX(sp_hash_layer_first(c, nullptr, eval_table.h, at.audit_ts.h, 0, cells, U(r_hash), U(r_multiset), L.audit.store.h, nullptr));
  } else {
    L.init = make_circuit_leaves(c, nullptr, eval_table.h, nullptr, 0, cells, r_hash, r_multiset);
    for (size_t k = 0; k < at.ops_addr.size(); k++) {
      L.read_vec.push_back(make_circuit_leaves(c, at.ops_addr[k].h, ops_val[k].h, at.read_ts[k].h, 0, n_ops, r_hash, r_multiset));
      L.write_vec.push_back(make_circuit_leaves(c, at.ops_addr[k].h, ops_val[k].h, at.read_ts[k].h, 1, n_ops, r_hash, r_multiset));
    }
    L.audit = make_circuit_leaves(c, nullptr, eval_table.h, at.audit_ts.h, 0, cells, r_hash, r_multiset);
  }
  // ProductCircuit::new (product_tree.rs:36-56) for every circuit
  std::vector<sp_table*> mem = {L.init.store.h, L.audit.store.h}, ops;
  for (auto& x : L.read_vec) ops.push_back(x.store.h);
  for (auto& x : L.write_vec) ops.push_back(x.store.h);
  SPX(sp_product_tree_many_from(c, mem.data(), mem.size(), cells, fuse ? 1 : 0));
  if (!ops.empty()) SPX(sp_product_tree_many_from(c, ops.data(), ops.size(), n_ops, fuse ? 1 : 0));
  return L;
}

// ProductLayerProof::prove (sparse_mlpoly.rs:1035-1214)
static ProductLayerProof product_layer_prove(sp_ctx* c, ProductLayer& row, ProductLayer& col, const MultiSparseMatPolynomialAsDense& dense,
                                             const Derefs& derefs, const FqVec& eval, Transcript& t, FqVec* rand_mem, FqVec* rand_ops) { HSPAN("product_layer_prove");
  t.append_protocol_name("Sparse polynomial product layer proof");
  ProductLayerProof P;
  auto side = [&](ProductLayer& L, Fq* init, FqVec* rd, FqVec* wr, Fq* audit, const char* li, const char* lr, const char* lw, const char* la) {
    std::vector<const ProductCircuit*> ps = {&L.init, &L.audit};
    for (auto& x : L.read_vec) ps.push_back(&x);
    for (auto& x : L.write_vec) ps.push_back(&x);
    FqVec ev = product_circuits_evaluate(c, ps);
    *init = ev[0];
    *audit = ev[1];
    for (size_t i = 0; i < L.read_vec.size(); i++) rd->push_back(ev[2 + i]);
    for (size_t i = 0; i < L.write_vec.size(); i++) wr->push_back(ev[2 + L.read_vec.size() + i]);
    Fq ws = fq_one(), rs = fq_one();
    for (auto& x : *wr) ws = ws * x;
    for (auto& x : *rd) rs = rs * x;
    REQUIRE(*init * ws == rs * *audit);  // multiset equality sanity check (:1057-1060, a live assert in the reference)
    t.append_scalar(li, *init);
    t.append_scalars(lr, *rd);
    t.append_scalars(lw, *wr);
    t.append_scalar(la, *audit);
  };
  side(row, &P.row_init, &P.row_read, &P.row_write, &P.row_audit, "claim_row_eval_init", "claim_row_eval_read", "claim_row_eval_write",
       "claim_row_eval_audit");
  side(col, &P.col_init, &P.col_read, &P.col_write, &P.col_audit, "claim_col_eval_init", "claim_col_eval_read", "claim_col_eval_write",
       "claim_col_eval_audit");
  size_t nb = derefs.row_ops_val.size();
  REQUIRE(eval.size() == nb && nb == 3);
  // dot-product circuits over clones (the sum-check binds them in place; the originals are evaluated again later)
  std::vector<DevTable> clones;
  clones.reserve(3 * nb);  // references into `clones` are taken below
  std::vector<DotProductCircuit> dl(nb), dr(nb);
  for (size_t i = 0; i < nb; i++) {
    clones.push_back(tab_clone(c, derefs.row_ops_val[i]));
    DevTable& cr = clones.back();
    clones.push_back(tab_clone(c, derefs.col_ops_val[i]));
    DevTable& cc = clones.back();
    clones.push_back(tab_clone(c, dense.val[i]));
    DevTable& cv = clones.back();
    size_t half = cr.len() / 2;  // DotProductCircuit::split (:90-109)
    dl[i] = DotProductCircuit{tab_view(c, cr, 0, half), tab_view(c, cc, 0, half), tab_view(c, cv, 0, half)};
    dr[i] = DotProductCircuit{tab_view(c, cr, half, half), tab_view(c, cc, half, half), tab_view(c, cv, half, half)};
  }
  {  // the six DotProductCircuit::evaluate (:84-88) in one launch; appended in the reference's order
    std::vector<const sp_table*> L6, R6, W6;
    for (size_t i = 0; i < nb; i++) {
      L6.push_back(dl[i].left.h); R6.push_back(dl[i].right.h); W6.push_back(dl[i].weight.h);
      L6.push_back(dr[i].left.h); R6.push_back(dr[i].right.h); W6.push_back(dr[i].weight.h);
    }
    FqVec v(2 * nb);
    SPX(sp_dot3_many(c, L6.data(), R6.data(), W6.data(), 2 * nb, dl[0].left.len(), U(v)));
    for (size_t i = 0; i < nb; i++) {
      const Fq &el = v[2 * i], &er = v[2 * i + 1];
      t.append_scalar("claim_eval_dotp_left", el);
      t.append_scalar("claim_eval_dotp_right", er);
      REQUIRE(el + er == eval[i]);
      P.eval_val[0].push_back(el);
      P.eval_val[1].push_back(er);
    }
  }
  std::vector<ProductCircuit*> ops = {&row.read_vec[0], &row.read_vec[1], &row.read_vec[2], &row.write_vec[0], &row.write_vec[1], &row.write_vec[2],
                                      &col.read_vec[0], &col.read_vec[1], &col.read_vec[2], &col.write_vec[0], &col.write_vec[1], &col.write_vec[2]};
  std::vector<DotProductCircuit*> dps = {&dl[0], &dr[0], &dl[1], &dr[1], &dl[2], &dr[2]};
  FqVec dps_evals = {P.eval_val[0][0], P.eval_val[1][0], P.eval_val[0][1], P.eval_val[1][1], P.eval_val[0][2], P.eval_val[1][2]};  // el, er of the same circuits
  FqVec ops_roots;  // the claims absorbed above, in the order of `ops`
  for (const FqVec* v : {&P.row_read, &P.row_write, &P.col_read, &P.col_write}) ops_roots.insert(ops_roots.end(), v->begin(), v->end());
  P.proof_ops = product_batched_prove(c, ops, dps, t, rand_ops, &dps_evals, &ops_roots);
  std::vector<ProductCircuit*> mem = {&row.init, &row.audit, &col.init, &col.audit};
  std::vector<DotProductCircuit*> none;
  FqVec mem_roots = {P.row_init, P.row_audit, P.col_init, P.col_audit};
  P.proof_mem = product_batched_prove(c, mem, none, t, rand_mem, nullptr, &mem_roots);
  return P;
}

// the n-to-1 reduction of DerefsEvalProof::prove_single (:79-121) and HashLayerProof::prove (:780-835): O(16) scalars
static Fq combine_n_to_one(FqVec evals, Transcript& t, const char* chal_label, const FqVec& r, FqVec* r_joint) {
  FqVec ch = t.challenge_vector(chal_label, log_2(evals.size()));
  for (size_t i = ch.size(); i-- > 0;) {  // bound_poly_var_bot (dense_mlpoly.rs:225-233)
    size_t n = evals.size() / 2;
    for (size_t k = 0; k < n; k++) evals[k] = evals[2 * k] + ch[i] * (evals[2 * k + 1] - evals[2 * k]);
    evals.resize(n);
  }
  REQUIRE(evals.size() == 1);
  *r_joint = ch;
  r_joint->insert(r_joint->end(), r.begin(), r.end());
  return evals[0];
}

// The ~23 DensePolynomial::evaluate calls of HashLayerProof::prove (sparse_mlpoly.rs:696-764) as <chi, T_k>, sharded by CONTIGUOUS CHUNKS
// (SURVEY 8e): shard g takes entries [g n/W, (g+1) n/W) of chi and of every table — views, nothing is copied — and the nt partial dot
// products per shard (32 * nt bytes) are exchanged and added; F_q sums are exact, the bytes are those of the unsharded evaluation.
// Virtual shards always; lock-step ranks from the configured table length (shard.cc: residue_min_log2).
static void dot_many_sharded(sp_ctx* c, sp_table* chi, const std::vector<sp_table*>& tabs, FqVec& out) {
  const size_t n = sp_table_len(chi), nt = tabs.size();
  std::vector<sp_ctx*> ctxs = commit_shard_residue_off(c) ? std::vector<sp_ctx*>() : residue_shard_ctxs(c);
  int rank = 0, world = 0, min_log2 = 64;
  size_t W = 0, me = 0;
  bool remote = false;
  if (ctxs.size() >= 2) W = ctxs.size();
  else if (!commit_shard_residue_off(c) && commit_shard_transport(c, &rank, &world, &min_log2) && min_log2 < 64 && n >= ((size_t)1 << min_log2)) {
    W = (size_t)world; me = (size_t)rank; remote = true; ctxs.assign(1, c);
  }
  if (W < 2 || n % W != 0 || n / W < 1024) { SPX(sp_dot_many(c, chi, const_cast<sp_table* const*>(tabs.data()), nt, U(out))); return; }
  const size_t per = n / W;
  if (!remote) SPX(sp_ctx_sync(c));  // the tables as produced by everything queued on the owning context
  FqVec all(W * nt);
  for (size_t g = 0; g < (remote ? 1 : W); g++) {
    const size_t sh = remote ? me : g;
    sp_ctx* cg = ctxs[g];
    sp_table* v = nullptr;
    SPX(sp_table_view(cg, chi, sh * per, per, &v));
    DevTable chi_v(cg, v);
    std::vector<DevTable> keep;
    std::vector<sp_table*> tv;
    for (sp_table* t : tabs) { SPX(sp_table_view(cg, t, sh * per, per, &v)); keep.emplace_back(cg, v); tv.push_back(v); }
    SPX(sp_dot_many(cg, chi_v.h, tv.data(), nt, all[sh * nt].l));
  }
  if (remote) commit_shard_gather(c, (uint8_t*)all.data(), 32 * nt);
  else commit_shard_note_gather(c, 32 * nt * W);
  for (size_t k = 0; k < nt; k++) {
    Fq acc = fq_zero();
    for (size_t g = 0; g < W; g++) acc += all[g * nt + k];
    out[k] = acc;
  }
}
// HashLayerProof::prove (sparse_mlpoly.rs:722-835)
static HashLayerProof hash_layer_prove(sp_ctx* c, const FqVec& rand_mem, const FqVec& rand_ops, const MultiSparseMatPolynomialAsDense& dense,
                                       const Derefs& derefs, const SparseMatPolyCommitmentGens& gens, Transcript& t, RandomTape& tape) { HSPAN("hash_layer_prove");
  t.append_protocol_name("Sparse polynomial hash layer proof");
  HashLayerProof H;
  // all DensePolynomial::evaluate(rand_ops) calls share chi(rand_ops); the audit polynomials share chi(rand_mem)
  DevTable chi_ops = tab_eq(c, rand_ops), chi_mem = tab_eq(c, rand_mem);
  std::vector<sp_table*> ops_tabs;
  for (auto& p : derefs.row_ops_val) ops_tabs.push_back(p.h);
  for (auto& p : derefs.col_ops_val) ops_tabs.push_back(p.h);
  for (auto& p : dense.row.ops_addr) ops_tabs.push_back(p.h);
  for (auto& p : dense.row.read_ts) ops_tabs.push_back(p.h);
  for (auto& p : dense.col.ops_addr) ops_tabs.push_back(p.h);
  for (auto& p : dense.col.read_ts) ops_tabs.push_back(p.h);
  for (auto& p : dense.val) ops_tabs.push_back(p.h);
  FqVec ev(ops_tabs.size());
  dot_many_sharded(c, chi_ops.h, ops_tabs, ev);
  std::vector<sp_table*> mem_tabs = {dense.row.audit_ts.h, dense.col.audit_ts.h};
  FqVec evm(2);
  dot_many_sharded(c, chi_mem.h, mem_tabs, evm);
  H.eval_derefs[0].assign(ev.begin(), ev.begin() + 3);
  H.eval_derefs[1].assign(ev.begin() + 3, ev.begin() + 6);
  {  // DerefsEvalProof::prove (:124-149)
    t.append_protocol_name("Derefs evaluation proof");
    FqVec evals = H.eval_derefs[0];
    evals.insert(evals.end(), H.eval_derefs[1].begin(), H.eval_derefs[1].end());
    evals.resize(next_pow2(evals.size()), fq_zero());
    t.append_scalars("evals_ops_val", evals);
    FqVec r_joint;
    Fq eval_joint = combine_n_to_one(evals, t, "challenge_combine_n_to_one", rand_ops, &r_joint);
    t.append_scalar("joint_claim_eval", eval_joint);
    H.proof_derefs = polyeval_prove(c, derefs.comb, nullptr, r_joint, eval_joint, nullptr, gens.gens_derefs, t, tape, nullptr);
  }
  H.row_addr.assign(ev.begin() + 6, ev.begin() + 9);
  H.row_read_ts.assign(ev.begin() + 9, ev.begin() + 12);
  H.col_addr.assign(ev.begin() + 12, ev.begin() + 15);
  H.col_read_ts.assign(ev.begin() + 15, ev.begin() + 18);
  H.eval_val.assign(ev.begin() + 18, ev.begin() + 21);
  H.row_audit_ts = evm[0];
  H.col_audit_ts = evm[1];
  FqVec evals_ops;
  evals_ops.insert(evals_ops.end(), H.row_addr.begin(), H.row_addr.end());
  evals_ops.insert(evals_ops.end(), H.row_read_ts.begin(), H.row_read_ts.end());
  evals_ops.insert(evals_ops.end(), H.col_addr.begin(), H.col_addr.end());
  evals_ops.insert(evals_ops.end(), H.col_read_ts.begin(), H.col_read_ts.end());
  evals_ops.insert(evals_ops.end(), H.eval_val.begin(), H.eval_val.end());
  evals_ops.resize(next_pow2(evals_ops.size()), fq_zero());
  t.append_scalars("claim_evals_ops", evals_ops);
  FqVec r_joint_ops;
  Fq joint_ops = combine_n_to_one(evals_ops, t, "challenge_combine_n_to_one", rand_ops, &r_joint_ops);
  t.append_scalar("joint_claim_eval_ops", joint_ops);
  H.proof_ops = polyeval_prove(c, dense.comb_ops, nullptr, r_joint_ops, joint_ops, nullptr, gens.gens_ops, t, tape, nullptr);
  FqVec evals_mem = {H.row_audit_ts, H.col_audit_ts};
  t.append_scalars("claim_evals_mem", evals_mem);
  FqVec r_joint_mem;
  Fq joint_mem = combine_n_to_one(evals_mem, t, "challenge_combine_two_to_one", rand_mem, &r_joint_mem);
  t.append_scalar("joint_claim_eval_mem", joint_mem);
  H.proof_mem = polyeval_prove(c, dense.comb_mem, nullptr, r_joint_mem, joint_mem, nullptr, gens.gens_mem, t, tape, nullptr);
  return H;
}

// The row half of `derefs` (row_ops_val of A, B, C: sparse_mlpoly.rs:506-513) depends on rx only, and rx is fixed by the
// FIRST sum-check of R1CSProof::prove. Its share of the derefs commitment — the largest MSM of the proof — is started on
// the context's background stream at that point and runs under the latency-bound second sum-check and the witness
// opening, whose kernels leave the chip almost idle and whose serial point encodes run on the host core.
struct DerefsEarly {
  FqVec rxe;
  DevTable mem_rx, comb;
  sp_job* job = nullptr;  // rows [0, rows_bg): the row half
  size_t rows_bg = 0;
  ~DerefsEarly() {
    if (job) { std::vector<uint8_t> sink(32 * rows_bg); (void)sp_job_wait(job, sink.data()); }
  }
};
static FqVec equalize_front(const FqVec& r, size_t len) {  // SparseMatPolyEvalProof::equalize (:1429-1445): zero-extend at the front
  if (r.size() >= len) return r;
  FqVec e(len - r.size(), fq_zero());
  e.insert(e.end(), r.begin(), r.end());
  return e;
}
static void derefs_early_begin(sp_ctx* c, const MultiSparseMatPolynomialAsDense& dense, const PolyCommitmentGens& gens_derefs, const FqVec& rx,
                               size_t ry_len, DerefsEarly* e) { HSPAN("derefs_early_begin");
  size_t N = dense.num_ops;
  e->rxe = equalize_front(rx, ry_len);
  e->mem_rx = tab_eq(c, e->rxe);
  if (e->mem_rx.len() != dense.num_mem_cells) { e->mem_rx = DevTable(); return; }  // sparse_eval_prove reports the mismatch
  e->comb = tab_alloc(c, next_pow2(6 * N));
  for (int k = 0; k < 3; k++) SPX(sp_gather(c, e->mem_rx.h, dense.row.ops_addr_usize[k].h, e->comb.h, k * N));
  size_t nv = log_2(e->comb.len()), Ls = pow2(nv / 2), Rs = pow2(nv - nv / 2);
  const MultiCommitGens& g = gens_derefs.gens.gens_n;
  size_t rows = 3 * N / Rs;  // rows of the L x R layout that hold row-half values only
  if (rows >= 64 && rows <= Ls && g.n() == Rs) {
    SPX(sp_commit_rows_dev_begin(c, g.g, g.G[0], e->comb.h, 0, rows, Rs, &e->job));
    e->rows_bg = rows;
  }
}

// SparseMatPolyEvalProof::prove (sparse_mlpoly.rs:1447-1514)
static SparseMatPolyEvalProof sparse_eval_prove(sp_ctx* c, const MultiSparseMatPolynomialAsDense& dense, const FqVec& rx, const FqVec& ry,
                                                const FqVec& evals, const SparseMatPolyCommitmentGens& gens, Transcript& t, RandomTape& tape,
                                                ProveTimes* tm, DerefsEarly* early = nullptr,
                                                const std::function<void()>* on_derefs_committed = nullptr) { HSPAN("sparse_eval_prove");
  t.append_protocol_name("Sparse polynomial evaluation proof");
  REQUIRE(evals.size() == dense.batch_size);
  FqVec rxe = rx, rye = ry;  // equalize (:1429-1445)
  if (rx.size() < ry.size()) { rxe.assign(ry.size() - rx.size(), fq_zero()); rxe.insert(rxe.end(), rx.begin(), rx.end()); }
  if (ry.size() < rx.size()) { rye.assign(rx.size() - ry.size(), fq_zero()); rye.insert(rye.end(), ry.begin(), ry.end()); }
  bool have_early = early && early->comb.h && early->rxe.size() == rxe.size();
  DevTable mem_rx = have_early ? std::move(early->mem_rx) : tab_eq(c, rxe), mem_ry = tab_eq(c, rye);
  REQUIRE(mem_rx.len() == dense.num_mem_cells);
  // Derefs (:506-513, :256-265, :47-61): six gathers written straight into the merged polynomial
  size_t N = dense.num_ops;
  Derefs derefs;
  if (have_early) derefs.comb = std::move(early->comb);
  else derefs.comb = tab_alloc(c, next_pow2(6 * N));
  for (int k = 0; k < 3; k++) {
    if (!have_early) SPX(sp_gather(c, mem_rx.h, dense.row.ops_addr_usize[k].h, derefs.comb.h, k * N));
    SPX(sp_gather(c, mem_ry.h, dense.col.ops_addr_usize[k].h, derefs.comb.h, (3 + k) * N));
  }
  for (int k = 0; k < 3; k++) derefs.row_ops_val.push_back(tab_view(c, derefs.comb, k * N, N));
  for (int k = 0; k < 3; k++) derefs.col_ops_val.push_back(tab_view(c, derefs.comb, (3 + k) * N, N));
  SparseMatPolyEvalProof P;
  double t0 = now_s();
  if (have_early && early->job) {  // rows [0, rows_bg) are in flight on the background stream: queue the rest here, then collect
    size_t nv = log_2(derefs.comb.len()), Ls = pow2(nv / 2), Rs = pow2(nv - nv / 2), r0 = early->rows_bg;
    const MultiCommitGens& g = gens.gens_derefs.gens.gens_n;
    std::vector<uint8_t> out(32 * Ls);
    // the rest of the rows on the main stream, without waiting: the background half finishes first, and its shares are
    // absorbed into the transcript (the order is C[0], C[1], ...: sparse_mlpoly.rs:204-210) while the main stream still works
    sp_job* jc = nullptr;
    // rows [6N / Rs, Ls) of the L x R layout are the zero padding of Derefs' merged polynomial (6N values in 2^ceil(log2 6N) slots: a
    // quarter of the rows at every size): an unblinded commitment to a zero row is the identity, whose encoding is 32 zero bytes (what
    // `out` already holds) — they are not launched, so the balanced MSM sees only rows that carry work
    size_t r1 = (6 * N + Rs - 1) / Rs;
    if (r1 > Ls || r1 <= r0 || (r1 - r0) % 256 != 0) r1 = Ls;
    if (r0 < Ls) {
      if (r1 - r0 > 8) SPX(sp_commit_rows_dev_start(c, g.g, g.G[0], g.h, derefs.comb.h, r0 * Rs, r1 - r0, Rs, nullptr, &jc));
      else SPX(sp_commit_rows_dev(c, g.g, g.G[0], g.h, derefs.comb.h, r0 * Rs, Ls - r0, Rs, nullptr, out.data() + 32 * r0));
    }
    struct JobGuard { sp_job*& j; size_t rows; ~JobGuard() { if (j) { std::vector<uint8_t> sink(32 * rows); (void)sp_job_wait(j, sink.data()); } } } guard{jc, r1 - r0};
    sp_job* j = early->job;
    early->job = nullptr;
    SPX(sp_job_wait(j, out.data()));
    P.comm_derefs.C.resize(Ls);
    t.append_message("derefs_commitment", "begin_derefs_commitment");                                // :204-210
    t.append_message("comm_poly_row_col_ops_val", "poly_commitment_begin");                          // append_poly_commitment, in two parts
    for (size_t i = 0; i < r0; i++) { P.comm_derefs.C[i] = to_cp(&out[32 * i]); t.append_point("poly_commitment_share", P.comm_derefs.C[i].data()); }
    if (jc) { j = jc; jc = nullptr; SPX(sp_job_wait(j, out.data() + 32 * r0)); }
    for (size_t i = r0; i < Ls; i++) { P.comm_derefs.C[i] = to_cp(&out[32 * i]); t.append_point("poly_commitment_share", P.comm_derefs.C[i].data()); }
    t.append_message("comm_poly_row_col_ops_val", "poly_commitment_end");
    t.append_message("derefs_commitment", "end_derefs_commitment");
  } else {
    P.comm_derefs = poly_commit(c, derefs.comb, log_2(derefs.comb.len()), gens.gens_derefs, nullptr);  // Derefs::commit (:64-67)
    t.append_message("derefs_commitment", "begin_derefs_commitment");                                  // :204-210
    append_poly_commitment(t, "comm_poly_row_col_ops_val", P.comm_derefs);
    t.append_message("derefs_commitment", "end_derefs_commitment");
  }
  if (tm) tm->commit_nondet_witness = now_s() - t0;
  if (on_derefs_committed) (*on_derefs_committed)();  // the last throughput-sized commitment of the proof is in: the next proof may start (ProofGate)
  FqVec r_mem_check = t.challenge_vector("challenge_r_hash", 2);
  double t1 = now_s();
  ProductLayer row = layers_new(c, mem_rx, dense.row, derefs.row_ops_val, r_mem_check[0], r_mem_check[1]);  // PolyEvalNetwork::new (:664-678)
  ProductLayer col = layers_new(c, mem_ry, dense.col, derefs.col_ops_val, r_mem_check[0], r_mem_check[1]);
  if (tm) tm->build_layered_network = now_s() - t1;
  double t2 = now_s();
  t.append_protocol_name("Sparse polynomial evaluation proof");  // PolyEvalNetworkProof::protocol_name (:1314-1316)
  FqVec rand_mem, rand_ops;
  P.proof_prod_layer = product_layer_prove(c, row, col, dense, derefs, evals, t, &rand_mem, &rand_ops);
  P.proof_hash_layer = hash_layer_prove(c, rand_mem, rand_ops, dense, derefs, gens, t, tape);
  if (tm) tm->evalproof_layered_network = now_s() - t2;
  return P;
}

// Several proofs in flight on ONE GPU (serving: one host thread + context per proof, bench.py `throughput_concurrent`). A proof is a
// throughput-bound first part (witness commitment ... derefs commitment: ~10 ms of which the row MSM fills ~8) followed by a latency-bound
// second part (the layered network's ~250 Fiat-Shamir trips, ~15 ms, the chip mostly idle). Two proofs started together collide in their
// first parts and idle together in their second. The gate (option host.proof_gate = 1) admits ONE proof at a time to the first part, in
// arrival order, so that the MSMs of proof k+1 run under the trips of proof k: a software pipeline over proofs. Off by default (a single
// proof never waits for it); each proof's bytes are what they are without it.
class ProofGate {
 public:
  void lock() {
    std::unique_lock<std::mutex> lk(m_);
    const uint64_t my = next_++;
    cv_.wait(lk, [&] { return serving_ == my; });
  }
  void unlock() {
    { std::lock_guard<std::mutex> lk(m_); serving_++; }
    cv_.notify_all();
  }
 private:
  std::mutex m_;
  std::condition_variable cv_;
  uint64_t next_ = 0, serving_ = 0;
};
// one gate per DEVICE: proofs on different GPUs of one process share no chip and must not wait for each other (ADVICE r4); a proof whose
// commitments are sharded over ranks never takes it (it would hold the gate across a collective)
static ProofGate& proof_gate_of(int dev) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<ProofGate>> gates;
  std::lock_guard<std::mutex> lk(mu);
  auto& g = gates[dev];
  if (!g) g.reset(new ProofGate());
  return *g;
}
struct ProofGateHold {  // released by hand when the derefs commitment is in (sparse_eval_prove), by the destructor on any other way out
  ProofGate* gate = nullptr;
  void acquire(sp_ctx* c) {
    if (ctx_opt(nullptr, "host.proof_gate") && !commit_shard_active(c)) { gate = &proof_gate_of(sp_ctx_device(c)); gate->lock(); }  // process-wide option
  }
  void release() { if (gate) { ProofGate* g = gate; gate = nullptr; g->unlock(); } }
  ~ProofGateHold() { release(); }
};

SNARK SNARK::prove(Ctx& ctx, const Instance& inst, const ComputationCommitment& comm, const ComputationDecommitment& decomm, const Fq* vars,
                   size_t nvars_given, const FqVec& inputs, const SNARKGens& gens, Transcript& t, const Fq* tape_seed, ProveTimes* tm,
                   const sp_table* vars_resident) {  // lib.rs:339-420
  if (gens.is_verifier_only()) throw Error("SNARK::prove: verifier-only generators have no fixed-base tables");
  double t0 = now_s();
  sp_ctx* c = ctx.h;
  SNARK P;
  {
  HSPAN("SNARK::prove");
  ProofGateHold gate;
  gate.acquire(c);
  Fq shared_seed;  // lock-step ranks of a sharded proof must share one tape: rank 0 draws it (shard.cc)
  if (!tape_seed && commit_shard_shared_seed(c, &shared_seed)) tape_seed = &shared_seed;
  RandomTape tape = tape_seed ? RandomTape("proof", *tape_seed) : RandomTape("proof");  // random.rs:11-18
  std::function<void()> prefix = [&]() {  // lib.rs:354-360; executed by r1cs_prove while the witness commitment is in flight
    t.append_protocol_name("Spartan SNARK proof");
    append_commitment(t, comm);
  };
  FqVec rx, ry;
  DerefsEarly early;
  size_t ry_len = log_2(inst.num_vars) + 1;  // R1CSProof::prove: num_rounds_y = log2(2 * num_vars) (r1csproof.rs:174)
  FqVec rx_seen;  // rx as handed to on_rx (r1cs_prove fills `rx` only when it returns)
  std::function<void(const FqVec&)> on_rx = [&](const FqVec& rx_now) {
    rx_seen = rx_now;
    derefs_early_begin(c, decomm.dense, gens.gens_r1cs_eval.gens_derefs, rx_now, ry_len, &early);
  };
  // R1CSInstance::evaluate (r1cs.rs:300-303) needs rx, ry and nothing else: queued on a low-priority stream when the second
  // sum-check ends, it runs in the idle time of the witness opening (launch-sized kernels, host trips) instead of standing on the
  // critical path behind it, next to the background MSM (1.04 -> ~0.1 ms for this span). Option overlap.eval_ahead = 0: the old place.
  struct EvalAhead {
    DevTable tx, ty;
    sp_job* job = nullptr;
    ~EvalAhead() { if (job) { uint8_t sink[96]; (void)sp_job_wait(job, sink); } }
  } ahead_eval;
  bool overlap = !commit_shard_active(c) && ctx_opt(c, "overlap.derefs") != 0;
  const bool eval_ahead = overlap && ctx_opt(c, "overlap.eval_ahead") != 0;
  std::function<void(const FqVec&)> on_ry = [&](const FqVec& ry_now) {
    if (eval_ahead) {
      ahead_eval.tx = tab_eq(c, rx_seen); ahead_eval.ty = tab_eq(c, ry_now);
      const sp_sparse* ms[3] = {inst.dA, inst.dB, inst.dC};
      SPX(sp_sparse_evaluate_begin(c, ms, 3, ahead_eval.tx.h, ahead_eval.ty.h, &ahead_eval.job));
    }
  };
  P.r1cs_sat_proof = r1cs_prove(c, inst, vars, nvars_given, inputs, gens.gens_r1cs_sat, t, tape, &rx, &ry, tm, overlap ? &on_rx : nullptr, &prefix,
                                eval_ahead ? &on_ry : nullptr, vars_resident);
  double t1 = now_s();
  if (ahead_eval.job) {
    sp_job* j = ahead_eval.job;
    ahead_eval.job = nullptr;
    uint8_t ev3[96];
    SPX(sp_job_wait(j, ev3));
    for (int k = 0; k < 3; k++) memcpy(P.inst_evals[k].l, ev3 + 32 * k, 32);
  } else {  // R1CSInstance::evaluate (r1cs.rs:300-303) -> multi_evaluate (sparse_mlpoly.rs:440-452)
    DevTable tx = tab_eq(c, rx), ty = tab_eq(c, ry);
    SPX(sp_sparse_evaluate(c, inst.dA, tx.h, ty.h, P.inst_evals[0].l));
    SPX(sp_sparse_evaluate(c, inst.dB, tx.h, ty.h, P.inst_evals[1].l));
    SPX(sp_sparse_evaluate(c, inst.dC, tx.h, ty.h, P.inst_evals[2].l));
  }
  t.append_scalar("Ar_claim", P.inst_evals[0]);
  t.append_scalar("Br_claim", P.inst_evals[1]);
  t.append_scalar("Cr_claim", P.inst_evals[2]);
  if (tm) tm->eval_sparse_polys = now_s() - t1;
  FqVec ev = {P.inst_evals[0], P.inst_evals[1], P.inst_evals[2]};
  std::function<void()> throughput_part_done = [&]() { gate.release(); };
  P.r1cs_eval_proof = sparse_eval_prove(c, decomm.dense, rx, ry, ev, gens.gens_r1cs_eval, t, tape, tm, &early, &throughput_part_done);  // r1cs.rs:326-349
  if (tm) tm->total = now_s() - t0;
  }
#ifdef SPZ_HOSTPROF
  HostSpan::dump();
  fprintf(stderr, "[hostprof] keccak permutations %llu, %.3f ms\n", (unsigned long long)keccak_prof().n, keccak_prof().t * 1e3);
  keccak_prof() = KeccakProf();
#endif
  g_calls.dump();
  return P;
}
