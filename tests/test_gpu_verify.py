"""NIZK::verify on the device (spartan_amd/host/verifier.cc over sp_eq_expand / sp_sparse_evaluate_begin / sp_msm_var / sp_commit_rows):
accepts what the HIP prover and the oracle's prover emit, agrees with the oracle's restated verifier on damaged proofs (and neither accepts
one), tells malformed bytes from wrong proofs, leaves a caller-owned transcript where the prover left it, and takes a handful of round trips."""
import ctypes
import pytest
from tests.helpers import *

pytestmark = pytest.mark.gpu
LABEL = b"nizk_example"


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


def oracle_bytes(orc, p):
    n = orc.orc_proof_bytes(p, None, sz(0))
    b = (ctypes.c_uint8 * n)()
    orc.orc_proof_bytes(p, b, sz(n))
    return bytes(b)


class Case:
    """a synthetic instance at 2^s on both sides (HIP driver and oracle) with the HIP prover's and the oracle's proof of it"""
    def __init__(self, P, ctx, orc, s, seed, digest=None):
        self.P, self.ctx, self.orc, self.s = P, ctx, orc, s
        N = self.N = 1 << s
        ni = self.ni = 10 if N > 16 else 1
        self.digest = digest if digest is not None else b"digest-%d" % s
        self.inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
        self.inst.set_digest(self.digest)
        self.gens = P.NIZKGens(ctx, N, N, ni)
        self.tape = P.seed_scalar(b"tape", seed)
        self.proof = P.NIZK.prove(ctx, self.inst, self.inst.vars, self.inst.inputs, self.gens, LABEL, self.tape)
        self.oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
        self.og = vp(orc.orc_nizk_gens_new(sz(N), sz(N), sz(ni)))
        self.op = vp(orc.orc_nizk_prove(self.oi, self.og, self.digest, sz(len(self.digest)), LABEL, self.tape, None))
        self.oproof = oracle_bytes(orc, self.op)

    def ours(self, b, label=LABEL, inputs=None):
        return self.P.NIZK.verify_status(self.ctx, self.inst, b, self.inst.inputs if inputs is None else inputs, self.gens, label)

    def oracle(self, b, label=LABEL):
        return self.orc.orc_nizk_verify_bytes(bytes(b), sz(len(b)), self.oi, self.og, self.digest, sz(len(self.digest)), label)

    def free(self):
        self.orc.orc_proof_free(self.op); self.orc.orc_nizk_gens_free(self.og); self.orc.orc_instance_free(self.oi)
        self.gens.free(); self.inst.free()


@pytest.fixture(scope="module")
def cases(P, ctx, orc):
    made = {}
    def get(s):
        if s not in made:
            made[s] = Case(P, ctx, orc, s, seed=s)
        return made[s]
    yield get
    for c in made.values():
        c.free()


# ---- accept
@pytest.mark.parametrize("s", [1, 2, 4, 7, 10, 13])
def test_accepts_hip_and_oracle_proofs(cases, s):
    c = cases(s)
    assert c.ours(c.proof) == 1
    assert c.ours(c.oproof) == 1
    assert c.oracle(c.proof) == 1
    assert c.P.NIZK.verify(c.ctx, c.inst, c.proof, c.inst.inputs, c.gens, LABEL) is True


def test_accepts_a_padded_instance(P, ctx, orc):
    """lib.rs:672-753 test_padded_constraints (num_cons = 1, num_vars = 0, num_inputs = 3), built as tests/test_gpu_proofs.py builds it"""
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
    inst.set_digest(b"padded")
    gens = P.NIZKGens(ctx, num_cons, num_vars, num_inputs)
    empty = (ctypes.c_uint64 * 0)()
    proof = P.NIZK.prove(ctx, inst, empty, inputs, gens, LABEL, P.seed_scalar(b"tape", 77))
    assert P.NIZK.verify_status(ctx, inst, proof, inputs, gens, LABEL) == 1
    assert P.NIZK.verify_status(ctx, inst, proof, mont_array([16, 1, 3]), gens, LABEL) == 0
    gens.free(); inst.free()


def test_accepts_a_proof_with_an_os_entropy_tape(cases):
    c = cases(7)
    fresh = c.P.NIZK.prove(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.gens, LABEL, None)
    assert fresh != c.proof and len(fresh) == len(c.proof)
    assert c.ours(fresh) == 1 and c.oracle(fresh) == 1


def test_verify_t_ends_where_prove_t_ends(cases):
    from tests.test_gpu_proofs import _caller_transcript_state
    c = cases(7)
    st_p, st_v = _caller_transcript_state(c.P.H, "spz_merlin_state"), _caller_transcript_state(c.P.H, "spz_merlin_state")
    proof = c.P.NIZK.prove_t(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.gens, st_p, c.tape)
    before = bytes(st_v)
    assert c.P.NIZK.verify_t(c.ctx, c.inst, proof, c.inst.inputs, c.gens, st_v) == 1
    assert bytes(st_v) == bytes(st_p) and bytes(st_v) != before
    assert c.ours(proof, label=b"caller protocol") == 0      # the earlier messages of the caller's transcript are bound into the proof


# ---- reject
def field_offsets(p):
    """{field name: byte offset} of an NIZK proof, walked from the struct layout (r1csproof.rs:21-37, sumcheck.rs:64-69, nizk/mod.rs:15-20,
    77-81, 146-152, 292-299, 421-428, bullet.rs:15-19, lib.rs:490-493): bincode has u64 lengths in front of every Vec and nothing else"""
    u64 = lambda o: int.from_bytes(p[o:o + 8], "little")
    f, o = {}, 0
    def vec(name, elem=32):
        nonlocal o
        k = u64(o); f[name] = o + 8; f[name + ".last"] = o + 8 + elem * (k - 1); o += 8 + elem * k
        return k
    def take(name, size=32):
        nonlocal o
        f[name] = o; o += size
    def zksc(tag):
        nonlocal o
        vec(tag + ".comm_polys"); vec(tag + ".comm_evals")
        k = u64(o); o += 8
        for i in range(k):
            take("%s.proofs[%d].delta" % (tag, i)); take("%s.proofs[%d].beta" % (tag, i)); vec("%s.proofs[%d].z" % (tag, i))
            take("%s.proofs[%d].z_delta" % (tag, i)); take("%s.proofs[%d].z_beta" % (tag, i))
    vec("comm_vars")
    zksc("sc1")
    for n in ("comm_Az", "comm_Bz", "comm_Cz", "comm_prod"):
        take("claims_phase2." + n)
    take("pok.alpha"); take("pok.z1"); take("pok.z2")
    take("prod.alpha"); take("prod.beta"); take("prod.delta")
    for i in range(5):
        take("prod.z[%d]" % i)
    take("eq1.alpha"); take("eq1.z")
    zksc("sc2")
    take("comm_vars_at_ry")
    vec("bullet.L_vec"); vec("bullet.R_vec")
    take("log.delta"); take("log.beta"); take("log.z1"); take("log.z2")
    take("eq2.alpha"); take("eq2.z")
    vec("rx"); vec("ry")
    assert o == len(p)
    return f


FLIPPED = ["comm_vars", "comm_vars.last", "sc1.comm_polys", "sc1.comm_evals.last", "sc1.proofs[0].z", "sc1.proofs[1].z.last", "sc1.proofs[0].delta",
           "claims_phase2.comm_Az", "claims_phase2.comm_Bz", "claims_phase2.comm_Cz", "claims_phase2.comm_prod",
           "pok.alpha", "pok.z1", "pok.z2", "prod.alpha", "prod.beta", "prod.delta", "prod.z[0]", "prod.z[4]", "eq1.alpha", "eq1.z",
           "sc2.comm_polys.last", "sc2.comm_evals", "sc2.proofs[0].z", "sc2.proofs[2].z_beta", "comm_vars_at_ry",
           "bullet.L_vec", "bullet.L_vec.last", "bullet.R_vec", "bullet.R_vec.last", "log.delta", "log.beta", "log.z1", "log.z2",
           "eq2.alpha", "eq2.z", "rx", "rx.last", "ry", "ry.last"]


def is_scalar(name):
    last = name[:-5].split(".")[-1] if name.endswith(".last") else name.split(".")[-1]
    return last in ("z", "z1", "z2", "z_beta", "z_delta", "rx", "ry") or last.startswith("z[")


def flip(orc, p, name, off):
    """one bit of the 32-byte field at `off` flipped. A scalar: bit 10. A point: the first bit, counted from bit 1 of byte 0, whose flip still
    DECODES (about every fourth does) — the oracle's verifier restates the reference's decompress().unwrap() as an abort, so it can only be asked
    about proofs whose points decode; undecodable points are test_undecodable_points_are_rejected_not_fatal's."""
    b = bytearray(p)
    if is_scalar(name):
        b[off + 1] ^= 4
        return bytes(b)
    out = (ctypes.c_uint8 * 32)()
    for k in range(1, 255):
        b[off + k // 8] ^= 1 << (k % 8)
        if orc.orc_pt_recompress(bytes(b[off:off + 32]), out) == 1:
            return bytes(b)
        b[off + k // 8] ^= 1 << (k % 8)
    raise AssertionError("no decodable neighbour of the point at %d" % off)


@pytest.mark.parametrize("s", [4, 10])
def test_one_flipped_bit_in_any_field_is_rejected_like_the_oracle_rejects_it(cases, orc, s):
    c = cases(s)
    offs = field_offsets(c.proof)
    for name in FLIPPED:
        bad = flip(orc, c.proof, name, offs[name])
        assert bad != c.proof and sum(bin(x ^ y).count("1") for x, y in zip(bad, c.proof)) == 1
        want, got = c.oracle(bad), c.ours(bad)
        assert (got == 1) == (want == 1), (name, got, want)
        assert got != 1 and want != 1, (name, got, want)


def test_undecodable_points_are_rejected_not_fatal(cases):
    """where the reference panics on a point of the proof that does not decode (dense_mlpoly.rs:382, r1csproof.rs:409, sumcheck.rs:131, the
    `?` of nizk/mod.rs) this verifier answers 0, and goes on working"""
    from tests.test_oracle_pins import RFC_BAD
    c = cases(4)
    offs = field_offsets(c.proof)
    bad_enc = bytes.fromhex(RFC_BAD[6])
    for name in FLIPPED:
        if is_scalar(name):
            continue
        o = offs[name]
        assert c.ours(c.proof[:o] + bad_enc + c.proof[o + 32:]) == 0, name
    assert c.ours(c.proof) == 1


def _add_one(p, off):
    """the scalar at `off` (raw Montgomery limbs) plus one: what orc_proof_tamper does to a field"""
    x = (int.from_bytes(p[off:off + 32], "little") + R) % Q
    return p[:off] + x.to_bytes(32, "little") + p[off + 32:]


@pytest.mark.parametrize("s", [4, 10])
def test_oracle_tampers_are_rejected(cases, orc, s):
    c = cases(s)
    offs = field_offsets(c.oproof)
    for what, name in ((0, "eq2.z"), (1, "sc1.proofs[0].z")):
        op = vp(orc.orc_nizk_prove(c.oi, c.og, c.digest, sz(len(c.digest)), LABEL, c.tape, None))
        orc.orc_proof_tamper(op, ctypes.c_int(what))
        assert orc.orc_nizk_verify(op, c.oi, c.og, c.digest, sz(len(c.digest)), LABEL) == 0
        orc.orc_proof_free(op)
        bad = _add_one(c.oproof, offs[name])          # the same change on the bytes
        assert c.oracle(bad) == 0 and c.ours(bad) == 0, name


@pytest.mark.parametrize("s", [4, 10])
def test_wrong_statement_is_rejected(P, ctx, orc, cases, s):
    c = cases(s)
    assert c.ours(c.proof, label=b"another_label") == 0 and c.oracle(c.proof, label=b"another_label") == 0
    # one changed input
    ins = from_mont_array(c.inst.inputs, c.ni)
    ins[-1] = (ins[-1] + 1) % Q
    assert c.ours(c.proof, inputs=mont_array(ins)) == 0
    # a wrong number of inputs is the caller's error (lib.rs:569), as Instance::is_sat reports it
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        c.ours(c.proof, inputs=mont_array(ins + [1]))
    # another digest
    c.inst.set_digest(b"another digest")
    try:
        assert c.ours(c.proof) == 0
    finally:
        c.inst.set_digest(c.digest)
    assert c.ours(c.proof) == 1
    # another instance of the same shape
    other = P.Instance.produce_synthetic_r1cs(ctx, c.N, c.N, c.ni, seed=1000 + s)
    other.set_digest(c.digest)
    assert P.NIZK.verify_status(ctx, other, c.proof, other.inputs, c.gens, LABEL) == 0
    assert P.NIZK.verify_status(ctx, other, c.proof, c.inst.inputs, c.gens, LABEL) == 0
    other.free()


@pytest.mark.parametrize("s", [4, 10])
def test_proof_from_a_wrong_witness_is_rejected(cases, s):
    c = cases(s)
    vars_ = from_mont_array(c.inst.vars, c.N)
    vars_[c.N // 3] = (vars_[c.N // 3] + 1) % Q
    wrong = mont_array(vars_)
    assert c.inst.is_sat(wrong, c.inst.inputs) is False
    proof = c.P.NIZK.prove(c.ctx, c.inst, wrong, c.inst.inputs, c.gens, LABEL, c.tape)
    assert len(proof) == len(c.proof)
    assert c.ours(proof) == 0 and c.oracle(proof) == 0


# ---- malformed
def test_malformed_bytes_are_told_apart_and_the_context_survives(cases):
    c = cases(4)
    for bad in (c.proof[:-1], c.proof[:len(c.proof) // 2], c.proof[:7], b"", c.proof + b"\x00", c.proof + c.proof):
        assert c.ours(bad) == -1
        assert c.P.NIZK.verify(c.ctx, c.inst, bad, c.inst.inputs, c.gens, LABEL) is False
    assert c.ours(c.proof) == 1


# ---- placement
def test_a_verification_is_a_handful_of_round_trips(cases):
    from spartan_amd import capi
    c = cases(13)
    raw = c.ctx.raw()
    assert c.ours(c.proof) == 1                                   # warm: the digest and the host-side generator tables exist
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
    print("round trips per NIZK::verify at 2^13:", trips, "launches:", {a: b for a, b in fam.items() if b})
    assert trips <= 8
    assert fam["msm_var"] == 1
