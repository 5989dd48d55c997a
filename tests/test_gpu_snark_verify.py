"""SNARK::verify on the device (spartan_amd/host/verifier.cc) against a Commitment loaded from bincode bytes: accepts what the HIP prover and
the oracle's prover emit, on synthetic instances and on the structured ones (num_ops != cells, non-square: equalize and uneven left / right
splits), agrees with the oracle's restated verifier on damaged proofs and commitments (and neither accepts one), answers 0 where the
reference would panic on an undecodable point, tells malformed bytes from wrong proofs, leaves a caller-owned transcript where the prover
left it, and sends the two commitments of the circuit through their resident point sets (sp_msm_points) and the proof's two through sp_msm_var."""
import ctypes
import pytest
from tests.helpers import *
from tests import structured_cases as sc
from tests import msm_var_cases as M
from tests.snark_layout import Layout

pytestmark = pytest.mark.gpu
LABEL = sc.SNARK_LABEL
SYNTHETIC = [1, 2, 4, 7, 10]
STRUCTURED = list(sc.SMALL)


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


def comm_header(cb):
    """(num_cons, num_vars, num_inputs, batch_size, num_ops, num_mem_cells) and the two share vectors of bincode(ComputationCommitment)"""
    h = [int.from_bytes(cb[8 * i:8 * i + 8], "little") for i in range(6)]
    n_ops = int.from_bytes(cb[48:56], "little")
    ops = cb[56:56 + 32 * n_ops]
    o = 56 + 32 * n_ops
    n_mem = int.from_bytes(cb[o:o + 8], "little")
    mem = cb[o + 8:o + 8 + 32 * n_mem]
    assert o + 8 + 32 * n_mem == len(cb)
    return h, ops, mem


class Case:
    """one instance on both sides with the HIP prover's and the oracle's SNARK of it, and the verifier's view: generators, a Commitment
    loaded from the bytes of serialize_commitment(), the inputs"""
    def __init__(self, P, ctx, orc, key):
        self.P, self.ctx, self.orc, self.key = P, ctx, orc, key
        if isinstance(key, int):
            N = 1 << key
            ni = 10 if N > 16 else 1
            self.inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=key)
            self.vars, self.inputs, self.n_inputs = self.inst.vars, self.inst.inputs, ni
            self.gens = P.SNARKGens(ctx, N, N, ni, N)
            self.tape = P.seed_scalar(b"tape", key)
            self.oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(key)))
            self.og = vp(orc.orc_snark_gens_new(sz(N), sz(N), sz(ni), sz(N)))
            self.oe = vp(orc.orc_snark_encode(self.oi, self.og))
            self.op = vp(orc.orc_snark_prove(self.oi, self.og, self.oe, LABEL, self.tape, None))
            self.oproof = sc.oracle_bytes(orc, orc.orc_proof_bytes, self.op)
            self.owned = True
        else:
            run = sc.oracle_run(orc, key)      # shared with tests/test_gpu_structured.py, left unchanged
            pk = run.pk
            self.inst = P.Instance.new(ctx, pk.num_cons, pk.num_vars, pk.num_inputs, pk.nnz, pk.rows, pk.cols, pk.vals)
            self.vars, self.inputs, self.n_inputs = pk.vars, pk.inputs, pk.num_inputs
            self.gens = P.SNARKGens(ctx, *run.gens_args)
            self.tape = P.seed_scalar(b"tape", sc.TAPE_SEED[key])
            self.oi, self.og, self.oe, self.op, self.oproof = run.oi, run.og, run.oe, run.op, run.snark
            self.owned = False
        self.enc = P.SNARK.encode(ctx, self.inst, self.gens)
        self.comm_bytes = self.enc.serialize_commitment()
        self.comm = P.Commitment.load(ctx, self.comm_bytes)
        self.proof = self.prove(self.vars, self.tape)

    def prove(self, vars_, tape):
        return self.P.SNARK.prove(self.ctx, self.inst, self.enc, vars_, self.inputs, self.gens, LABEL, tape)

    def ours(self, b, label=LABEL, inputs=None, comm=None):
        return self.P.SNARK.verify_status(self.ctx, comm or self.comm, b, self.inputs if inputs is None else inputs, self.gens, label)

    def oracle(self, b, label=LABEL, inputs=None, comm_bytes=None):
        h, ops, mem = comm_header(comm_bytes or self.comm_bytes)
        return self.orc.orc_snark_verify_bytes(bytes(b), sz(len(b)), self.og, sz(h[0]), sz(h[1]), sz(h[2]), sz(h[4]), sz(h[5]), ops, sz(len(ops) // 32),
                                               mem, sz(len(mem) // 32), self.inputs if inputs is None else inputs, label)

    def free(self):
        if self.owned:
            self.orc.orc_proof_free(self.op); self.orc.orc_encode_free(self.oe); self.orc.orc_snark_gens_free(self.og); self.orc.orc_instance_free(self.oi)
        self.comm.free(); self.enc.free(); self.gens.free(); self.inst.free()


@pytest.fixture(scope="module")
def cases(P, ctx, orc):
    made = {}
    def get(key):
        if key not in made:
            made[key] = Case(P, ctx, orc, key)
        return made[key]
    yield get
    for c in made.values():
        c.free()


# ---- accept
@pytest.mark.parametrize("key", SYNTHETIC + STRUCTURED)
def test_accepts_hip_and_oracle_proofs(cases, key):
    c = cases(key)
    assert c.ours(c.proof) == 1
    assert c.ours(c.oproof) == 1
    assert c.oracle(c.proof) == 1
    assert c.P.SNARK.verify(c.ctx, c.comm, c.proof, c.inputs, c.gens, LABEL) is True


def test_commitment_of_an_encoding_is_the_one_loaded_from_its_bytes(cases):
    c = cases(4)
    comm = c.enc.commitment(c.ctx)
    assert c.ours(c.proof, comm=comm) == 1
    comm.free()


def test_accepts_a_padded_instance(P, ctx, orc):
    """lib.rs:672-753 test_padded_constraints (num_cons = 1, num_vars = 0, num_inputs = 3), built as tests/test_gpu_verify.py builds it"""
    num_cons, num_vars, num_inputs = 1, 0, 3
    le = lambda x: (x % Q).to_bytes(32, "little")
    A = [(0, num_vars + 2, le(1))]
    B = [(0, num_vars + 2, le(1))]
    C = [(0, num_vars + 1, le(1)), (0, num_vars, le(-13)), (0, num_vars + 3, le(-1))]
    nnz = [len(A), len(B), len(C)]
    ent = A + B + C
    rows = (ctypes.c_uint64 * len(ent))(*[e[0] for e in ent]); cols = (ctypes.c_uint64 * len(ent))(*[e[1] for e in ent])
    vals = b"".join(e[2] for e in ent)
    inputs = mont_array([16, 1, 2])
    inst = P.Instance.new(ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals)
    inst.num_inputs = num_inputs
    gens = P.SNARKGens(ctx, num_cons, num_vars, num_inputs, 3)
    enc = P.SNARK.encode(ctx, inst, gens)
    comm = enc.commitment(ctx)
    empty = (ctypes.c_uint64 * 0)()
    proof = P.SNARK.prove(ctx, inst, enc, empty, inputs, gens, LABEL, P.seed_scalar(b"tape", 77))
    assert P.SNARK.verify_status(ctx, comm, proof, inputs, gens, LABEL) == 1
    assert P.SNARK.verify_status(ctx, comm, proof, mont_array([16, 1, 3]), gens, LABEL) == 0
    comm.free(); enc.free(); gens.free(); inst.free()


def test_accepts_a_proof_with_an_os_entropy_tape(cases):
    c = cases(7)
    fresh = c.prove(c.vars, None)
    assert fresh != c.proof and len(fresh) == len(c.proof)
    assert c.ours(fresh) == 1 and c.oracle(fresh) == 1


def test_verify_t_ends_where_prove_t_ends(cases):
    from tests.test_gpu_proofs import _caller_transcript_state
    c = cases(7)
    st_p, st_v = _caller_transcript_state(c.P.H, "spz_merlin_state"), _caller_transcript_state(c.P.H, "spz_merlin_state")
    proof = c.P.SNARK.prove_t(c.ctx, c.inst, c.enc, c.vars, c.inputs, c.gens, st_p, c.tape)
    before = bytes(st_v)
    assert c.P.SNARK.verify_t(c.ctx, c.comm, proof, c.inputs, c.gens, st_v) == 1
    assert bytes(st_v) == bytes(st_p) and bytes(st_v) != before
    assert c.ours(proof, label=b"caller protocol") == 0      # the earlier messages of the caller's transcript are bound into the proof


# ---- reject
# at least one field of every struct of the proof (tests/snark_layout.py names them), the first and last element of every vector that does
# not sit inside a repeated struct; of the repeated ones (sum-check rounds, layers) the first, a middle and a late one
FLIPPED = [
    "comm_vars", "comm_vars.last",
    "sc1.comm_polys", "sc1.comm_polys.last", "sc1.comm_evals", "sc1.comm_evals.last", "sc1.proofs[0].delta", "sc1.proofs[0].beta", "sc1.proofs[0].z",
    "sc1.proofs[0].z.last", "sc1.proofs[1].z_delta", "sc1.proofs[1].z_beta",
    "claims_phase2.comm_Az", "claims_phase2.comm_Bz", "claims_phase2.comm_Cz", "claims_phase2.comm_prod",
    "pok.alpha", "pok.z1", "pok.z2", "prod.alpha", "prod.beta", "prod.delta", "prod.z[0]", "prod.z[4]", "eq1.alpha", "eq1.z",
    "sc2.comm_polys", "sc2.comm_polys.last", "sc2.comm_evals", "sc2.comm_evals.last", "sc2.proofs[0].z", "sc2.proofs[2].z.last", "sc2.proofs[2].z_beta",
    "comm_vars_at_ry", "eval_vars.L_vec", "eval_vars.L_vec.last", "eval_vars.R_vec", "eval_vars.R_vec.last", "eval_vars.delta", "eval_vars.beta",
    "eval_vars.z1", "eval_vars.z2", "eq2.alpha", "eq2.z",
    "inst_evals.A", "inst_evals.B", "inst_evals.C",
    "comm_derefs", "comm_derefs.last",
    "prod_layer.row_init", "prod_layer.row_read", "prod_layer.row_read.last", "prod_layer.row_write", "prod_layer.row_write.last", "prod_layer.row_audit",
    "prod_layer.col_init", "prod_layer.col_read", "prod_layer.col_read.last", "prod_layer.col_write", "prod_layer.col_write.last", "prod_layer.col_audit",
    "prod_layer.eval_val_left", "prod_layer.eval_val_left.last", "prod_layer.eval_val_right", "prod_layer.eval_val_right.last",
    "proof_mem.proof[0].claims_prod_left", "proof_mem.proof[0].claims_prod_right.last", "proof_mem.proof[1].compressed_polys[0]",
    "proof_mem.proof[1].compressed_polys[0].last", "proof_mem.proof[2].compressed_polys[1]", "proof_mem.proof[2].claims_prod_left.last",
    "proof_mem.proof[2].claims_prod_right",
    "proof_ops.proof[0].claims_prod_left", "proof_ops.proof[0].claims_prod_left.last", "proof_ops.proof[1].compressed_polys[0]",
    "proof_ops.proof[2].compressed_polys[1].last", "proof_ops.proof[2].claims_prod_right", "proof_ops.proof[2].claims_prod_right.last",
    "proof_ops.claims_dotp_left", "proof_ops.claims_dotp_left.last", "proof_ops.claims_dotp_right", "proof_ops.claims_dotp_right.last",
    "proof_ops.claims_dotp_weight", "proof_ops.claims_dotp_weight.last",
    "hash_layer.row_addr", "hash_layer.row_addr.last", "hash_layer.row_read_ts", "hash_layer.row_read_ts.last", "hash_layer.row_audit_ts",
    "hash_layer.col_addr", "hash_layer.col_addr.last", "hash_layer.col_read_ts", "hash_layer.col_read_ts.last", "hash_layer.col_audit_ts",
    "hash_layer.eval_val", "hash_layer.eval_val.last", "hash_layer.eval_row_ops_val", "hash_layer.eval_row_ops_val.last",
    "hash_layer.eval_col_ops_val", "hash_layer.eval_col_ops_val.last",
    "hash_layer.proof_ops.L_vec", "hash_layer.proof_ops.L_vec.last", "hash_layer.proof_ops.R_vec", "hash_layer.proof_ops.R_vec.last",
    "hash_layer.proof_ops.delta", "hash_layer.proof_ops.beta", "hash_layer.proof_ops.z1", "hash_layer.proof_ops.z2",
    "hash_layer.proof_mem.L_vec", "hash_layer.proof_mem.L_vec.last", "hash_layer.proof_mem.R_vec", "hash_layer.proof_mem.R_vec.last",
    "hash_layer.proof_mem.delta", "hash_layer.proof_mem.beta", "hash_layer.proof_mem.z1", "hash_layer.proof_mem.z2",
    "hash_layer.proof_derefs.L_vec", "hash_layer.proof_derefs.L_vec.last", "hash_layer.proof_derefs.R_vec", "hash_layer.proof_derefs.R_vec.last",
    "hash_layer.proof_derefs.delta", "hash_layer.proof_derefs.beta", "hash_layer.proof_derefs.z1", "hash_layer.proof_derefs.z2",
]


def flip(orc, p, off, kind):
    """one bit of the 32-byte field at `off` flipped. A scalar: bit 10. A point: the first bit, counted from bit 1 of byte 0, whose flip still
    DECODES — the oracle's verifier restates the reference's decompress().unwrap() as an abort, so it can only be asked about proofs whose
    points decode; undecodable points are test_undecodable_points_are_rejected_not_fatal's."""
    b = bytearray(p)
    if kind == "scalar":
        b[off + 1] ^= 4
        return bytes(b)
    out = (ctypes.c_uint8 * 32)()
    for k in range(1, 255):
        b[off + k // 8] ^= 1 << (k % 8)
        if orc.orc_pt_recompress(bytes(b[off:off + 32]), out) == 1:
            return bytes(b)
        b[off + k // 8] ^= 1 << (k % 8)
    raise AssertionError("no decodable neighbour of the point at %d" % off)


def check_flips(c, orc, names):
    lay = Layout(c.proof)
    visited = []
    for name in names:
        off, kind = lay.fields[name]          # a KeyError is a listed field that this proof does not have: none may be skipped
        bad = flip(orc, c.proof, off, kind)
        assert bad != c.proof and sum(bin(x ^ y).count("1") for x, y in zip(bad, c.proof)) == 1
        want, got = c.oracle(bad), c.ours(bad)
        assert got != 1 and want != 1, (name, got, want)
        assert got == want, (name, got, want)
        visited.append(name)
    assert visited == list(names) and len(set(visited)) == len(visited)
    assert c.ours(c.proof) == 1


@pytest.mark.parametrize("key", [4, 10, "shifted"])
def test_one_flipped_bit_in_any_listed_field_is_rejected_like_the_oracle_rejects_it(cases, orc, key):
    check_flips(cases(key), orc, FLIPPED)


def test_one_flipped_bit_in_the_ends_of_every_vector_at_2_4(cases, orc):
    """every vector the layout finds, inside the repeated structs too: its first and its last element"""
    c = cases(4)
    lay = Layout(c.proof)
    vecs = [n for _, _, n in lay.lengths if n in lay.fields]
    names = [n for v in vecs for n in (v, v + ".last")]
    assert len(vecs) >= 60
    check_flips(c, orc, names)


def _add_one(p, off):
    """the scalar at `off` (raw Montgomery limbs) plus one: what orc_proof_tamper does to a field"""
    x = (int.from_bytes(p[off:off + 32], "little") + R) % Q
    return p[:off] + x.to_bytes(32, "little") + p[off + 32:]


@pytest.mark.parametrize("key", [4, 10])
def test_oracle_tampers_are_rejected(cases, orc, key):
    c = cases(key)
    lay = Layout(c.oproof)
    for what, name in ((0, "eq2.z"), (1, "sc1.proofs[0].z"), (2, "inst_evals.A"), (3, "hash_layer.eval_val")):
        op = vp(orc.orc_snark_prove(c.oi, c.og, c.oe, LABEL, c.tape, None))
        orc.orc_proof_tamper(op, ctypes.c_int(what))
        assert orc.orc_snark_verify(op, c.oi, c.og, c.oe, LABEL) == 0
        orc.orc_proof_free(op)
        bad = _add_one(c.oproof, lay.fields[name][0])          # the same change on the bytes
        assert c.oracle(bad) == 0 and c.ours(bad) == 0, name


@pytest.mark.parametrize("key", [4, 10, "ops_heavy"])
def test_wrong_statement_is_rejected(P, cases, key):
    c = cases(key)
    assert c.ours(c.proof, label=b"another_label") == 0 and c.oracle(c.proof, label=b"another_label") == 0
    ins = from_mont_array(c.inputs, c.n_inputs)
    ins[-1] = (ins[-1] + 1) % Q
    assert c.ours(c.proof, inputs=mont_array(ins)) == 0 and c.oracle(c.proof, inputs=mont_array(ins)) == 0
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):      # lib.rs:437: the caller's error
        c.ours(c.proof, inputs=mont_array(ins + [1]))
    assert c.ours(c.proof) == 1


@pytest.mark.parametrize("key", [4, 10])
def test_proof_from_a_wrong_witness_is_rejected(cases, key):
    c = cases(key)
    N = 1 << key
    vars_ = from_mont_array(c.vars, N)
    vars_[N // 3] = (vars_[N // 3] + 1) % Q
    wrong = mont_array(vars_)
    assert c.inst.is_sat(wrong, c.inputs) is False
    proof = c.prove(wrong, c.tape)
    assert len(proof) == len(c.proof)
    assert c.ours(proof) == 0 and c.oracle(proof) == 0


@pytest.mark.parametrize("key", [4, 10])
def test_wrong_commitment_is_rejected(P, ctx, orc, cases, key):
    c = cases(key)
    N = 1 << key
    # another instance of the same shape
    other = P.Instance.produce_synthetic_r1cs(ctx, N, N, c.n_inputs, seed=1000 + key)
    oenc = P.SNARK.encode(ctx, other, c.gens)
    ob = oenc.serialize_commitment()
    assert ob != c.comm_bytes and len(ob) == len(c.comm_bytes)
    ocomm = P.Commitment.load(ctx, ob)
    assert c.ours(c.proof, comm=ocomm) == 0 and c.oracle(c.proof, comm_bytes=ob) == 0
    ocomm.free(); oenc.free(); other.free()
    # one share swapped for another decodable point: the first and the last share of either vector
    _, ops, mem = comm_header(c.comm_bytes)
    stranger = M.points(orc, 1, seed=7)[0]
    for off in (56, 56 + len(ops) - 32, 56 + len(ops) + 8, len(c.comm_bytes) - 32):
        sb = c.comm_bytes[:off] + stranger + c.comm_bytes[off + 32:]
        swapped = P.Commitment.load(ctx, sb)
        assert c.ours(c.proof, comm=swapped) == 0 and c.oracle(c.proof, comm_bytes=sb) == 0, off
        swapped.free()
    assert c.ours(c.proof) == 1


def test_undecodable_points_are_rejected_not_fatal(P, ctx, cases):
    """where the reference panics on a point of the proof that does not decode (decompress().unwrap()) this verifier answers 0 and goes on
    working: every point of the proof at 2^4 in turn, every element of every vector of points included; an undecodable share of the
    commitment is found once, when it is loaded"""
    from tests.test_oracle_pins import RFC_BAD
    c = cases(4)
    lay = Layout(c.proof)
    in_vectors = {v for v in lay.vectors} | {v + ".last" for v in lay.vectors}
    points = [(n, o) for n, (o, kind) in lay.fields.items() if kind == "point" and n not in in_vectors]
    points += [("%s[%d]" % (v, i), o + 32 * i) for v, (o, k, kind) in lay.vectors.items() if kind == "point" for i in range(k)]   # every element
    assert len(points) >= 80 and len({o for _, o in points}) == len(points)
    for k, (name, o) in enumerate(points):
        bad_enc = bytes.fromhex(RFC_BAD[k % len(RFC_BAD)])
        assert c.ours(c.proof[:o] + bad_enc + c.proof[o + 32:]) == 0, name
    assert c.ours(c.proof) == 1
    _, ops, _ = comm_header(c.comm_bytes)
    for off in (56, 56 + len(ops) - 32, 56 + len(ops) + 8, len(c.comm_bytes) - 32):
        with pytest.raises(P.SpartanHipError, match="sp_points_upload"):
            P.Commitment.load(ctx, c.comm_bytes[:off] + bytes.fromhex(RFC_BAD[6]) + c.comm_bytes[off + 32:])
    with pytest.raises(P.SpartanHipError, match="malformed"):
        P.Commitment.load(ctx, c.comm_bytes[:-1])
    assert c.ours(c.proof) == 1


# ---- malformed
def test_malformed_bytes_are_told_apart_and_the_context_survives(cases):
    c = cases(4)
    for bad in (c.proof[:-1], c.proof[:len(c.proof) // 2], c.proof[:7], b"", c.proof + b"\x00", c.proof + c.proof):
        assert c.ours(bad) == -1
        assert c.P.SNARK.verify(c.ctx, c.comm, bad, c.inputs, c.gens, LABEL) is False
    assert c.ours(c.proof) == 1


# ---- placement
def test_placement_of_a_verification_at_2_10(cases):
    """the proof's two commitments (comm_vars, comm_derefs) go through sp_msm_var, the circuit's two through their resident point sets; and the
    count of round trips is the one DESIGN.md section 3 takes apart"""
    from spartan_amd import capi
    c = cases(10)
    raw = c.ctx.raw()
    assert c.ours(c.proof) == 1                                   # warm: the host-side generator tables exist
    L = capi.lib
    assert L.sp_prof_enable(raw, ctypes.c_int(1)) == 0 and L.sp_prof_reset(raw) == 0
    t0 = L.sp_ctx_trips(raw)
    assert c.ours(c.proof) == 1
    trips = L.sp_ctx_trips(raw) - t0
    cap = 64
    names = (ctypes.c_char_p * cap)(); ms = (ctypes.c_double * cap)(); n = (ctypes.c_uint64 * cap)(); by = (ctypes.c_double * cap)()
    k = L.sp_prof_read(raw, names, ms, n, by, ctypes.c_int(cap))
    L.sp_prof_enable(raw, ctypes.c_int(0))
    fam = {names[i].decode(): int(n[i]) for i in range(k)}
    print("round trips per SNARK::verify at 2^10:", trips, "launches:", {a: b for a, b in fam.items() if b})
    assert fam["msm_var"] == 2 and fam["msm_points"] == 2
    assert trips <= 8      # 4 C_LZ (2 sp_msm_var, 2 sp_msm_points) + 4 G_hat (sp_commit_rows), one per PolyEvalProof
