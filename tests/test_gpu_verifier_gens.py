"""Verifier-only generators (SNARKGens.verifier_only / NIZKGens.verifier_only; spartan_amd/host/verifier.cc): the generator streams held as
resident point sets (sp_points_from_uniform), without the prover's fixed-base window tables. Under them SNARK::verify, NIZK::verify and both
verify_many give, proof for proof, the verdict they give under the prover's generators, which is the oracle's: G_hat goes through
sp_msm_points_range over gens_n's range of the stream (sp_msm_points_range_many behind the gate), the few-term combinations through the host
tables of the set. Accepted and damaged proofs, wrong statements, malformed bytes, caller-owned transcripts, the bytes held, and the refusal
of everything that needs the prover's tables."""
import ctypes
import pytest
from tests.helpers import *
from tests import structured_cases as sc
from tests.snark_layout import Layout
from tests.test_gpu_snark_verify import Case as SnarkCase, flip
from tests.test_gpu_verify import Case as NizkCase, field_offsets, is_scalar, FLIPPED as NIZK_FLIPPED

pytestmark = pytest.mark.gpu
LABEL = sc.SNARK_LABEL
NIZK_LABEL = b"nizk_example"
SYNTHETIC = [1, 2, 4, 7, 10, 12]      # 2^12: the `ops` and `derefs` openings are exactly one full 256-point block
STRUCTURED = list(sc.SMALL)
# one field in each top-level region of the proof (the part of a tests/snark_layout.Layout name before its first dot), and in the regions that
# hold a PolyEvalProof the fields its last equation takes next to G_hat
REGIONS = ["comm_vars", "sc1", "claims_phase2", "pok", "prod", "eq1", "sc2", "comm_vars_at_ry", "eval_vars", "eq2", "inst_evals", "comm_derefs",
           "prod_layer", "proof_mem", "proof_ops", "hash_layer"]
NEXT_TO_G_HAT = ["eval_vars.L_vec", "eval_vars.R_vec.last", "eval_vars.z1", "hash_layer.proof_ops.L_vec", "hash_layer.proof_ops.z1",
                 "hash_layer.proof_mem.R_vec", "hash_layer.proof_mem.z2", "hash_layer.proof_derefs.L_vec.last", "hash_layer.proof_derefs.z1"]


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


def stream_points(gens_args):
    """points of the two generator streams of SNARKGens::new(num_cons, num_vars, num_inputs, nnz) (lib.rs:288-307)"""
    num_cons, num_vars, num_inputs, nnz = gens_args
    p2 = lambda n: 1 << max(n - 1, 0).bit_length()
    lg = lambda n: max(n - 1, 0).bit_length()
    nvp = p2(max(num_vars, num_inputs + 1))
    sat = max((1 << (lg(nvp) - lg(nvp) // 2)) + 2, 5)
    v_ops, v_mem, v_derefs = lg(p2(nnz)) + 4, max(lg(num_cons), lg(2 * nvp)) + 1, lg(p2(nnz)) + 3
    return sat, max(1 << (v - v // 2) for v in (v_ops, v_mem, v_derefs)) + 2


class Snark(SnarkCase):
    """the case of tests/test_gpu_snark_verify.py (instance, prover generators, commitment, the HIP prover's and the oracle's proof) with the
    verifier-only generators of the same shape next to it"""
    def __init__(self, P, ctx, orc, key):
        super().__init__(P, ctx, orc, key)
        N = 1 << key if isinstance(key, int) else None
        self.gens_args = (N, N, self.n_inputs, N) if N else tuple(sc.oracle_run(orc, key).gens_args)
        self.vg = P.SNARKGens.verifier_only(ctx, *self.gens_args)

    def light(self, b, label=LABEL, inputs=None):
        return self.P.SNARK.verify_status(self.ctx, self.comm, b, self.inputs if inputs is None else inputs, self.vg, label)

    def free(self):
        self.vg.free()
        super().free()


class Nizk(NizkCase):
    def __init__(self, P, ctx, orc, s):
        super().__init__(P, ctx, orc, s, seed=s)
        self.vg = P.NIZKGens.verifier_only(ctx, self.N, self.N, self.ni)

    def light(self, b, label=NIZK_LABEL, inputs=None):
        return self.P.NIZK.verify_status(self.ctx, self.inst, b, self.inst.inputs if inputs is None else inputs, self.vg, label)

    def free(self):
        self.vg.free()
        super().free()


def _cache(make):
    made = {}
    def get(key):
        if key not in made:
            made[key] = make(key)
        return made[key]
    return made, get


@pytest.fixture(scope="module")
def snarks(P, ctx, orc):
    made, get = _cache(lambda key: Snark(P, ctx, orc, key))
    yield get
    for c in made.values():
        c.free()


@pytest.fixture(scope="module")
def nizks(P, ctx, orc):
    made, get = _cache(lambda s: Nizk(P, ctx, orc, s))
    yield get
    for c in made.values():
        c.free()


# ---- accept
@pytest.mark.parametrize("key", SYNTHETIC + STRUCTURED)
def test_snark_accepts_hip_and_oracle_proofs(snarks, key):
    c = snarks(key)
    assert c.vg.is_verifier_only and not c.gens.is_verifier_only
    assert c.light(c.proof) == 1
    assert c.light(c.oproof) == 1
    assert c.P.SNARK.verify(c.ctx, c.comm, c.proof, c.inputs, c.vg, LABEL) is True
    for which in (0, 1):
        assert c.vg.stream(which) == c.gens.stream(which)
    sat, ev = stream_points(c.gens_args)
    assert (len(c.vg.stream(0)), len(c.vg.stream(1))) == (32 * sat, 32 * ev)
    assert c.vg.resident_bytes() == 65536 * (sat + ev)


@pytest.mark.parametrize("s", SYNTHETIC)
def test_nizk_accepts_hip_and_oracle_proofs(nizks, s):
    c = nizks(s)
    assert c.vg.is_verifier_only and not c.gens.is_verifier_only
    assert c.light(c.proof) == 1
    assert c.light(c.oproof) == 1
    assert c.P.NIZK.verify(c.ctx, c.inst, c.proof, c.inst.inputs, c.vg, NIZK_LABEL) is True
    sat, _ = stream_points((c.N, c.N, c.ni, 1))
    assert c.vg.resident_bytes() == 65536 * sat


# ---- reject: the verdict under verifier-only generators is the one under the prover's, which is the oracle's, and none is an accept
def snark_flips(c, orc):
    lay = Layout(c.proof)
    names = list(dict.fromkeys([next(n for n in lay.fields if n == r or n.startswith(r + ".")) for r in REGIONS] + NEXT_TO_G_HAT))
    assert {n.split(".")[0] for n in names} == set(REGIONS)
    return [(n, flip(orc, c.proof, *lay.fields[n])) for n in names]


@pytest.mark.parametrize("key", [4, 7])
def test_snark_flipped_regions_are_rejected_alike(snarks, orc, key):
    c = snarks(key)
    for name, bad in snark_flips(c, orc):
        got, full, want = c.light(bad), c.ours(bad), c.oracle(bad)
        assert got == full == want and got != 1, (name, got, full, want)
    assert c.light(c.proof) == 1


@pytest.mark.parametrize("s", [4, 7])
def test_nizk_flipped_fields_are_rejected_alike(nizks, orc, s):
    c = nizks(s)
    f = field_offsets(c.proof)
    for name in NIZK_FLIPPED:        # every region of the proof (tests/test_gpu_verify.py)
        bad = flip(orc, c.proof, f[name], "scalar" if is_scalar(name) else "point")
        got, full, want = c.light(bad), c.ours(bad), c.oracle(bad)
        assert got == full == want and got != 1, (name, got, full, want)
    assert c.light(c.proof) == 1


@pytest.mark.parametrize("key", [4, 7])
def test_snark_wrong_statement_and_malformed_bytes(P, snarks, key):
    c = snarks(key)
    ins = from_mont_array(c.inputs, c.n_inputs)
    ins[-1] = (ins[-1] + 1) % Q
    wrong = mont_array(ins)
    assert c.light(c.proof, inputs=wrong) == c.ours(c.proof, inputs=wrong) == c.oracle(c.proof, inputs=wrong) == 0
    other = b"another_label"
    assert c.light(c.proof, label=other) == c.ours(c.proof, label=other) == c.oracle(c.proof, label=other) == 0
    for bad in (c.proof[:-1], c.proof[:len(c.proof) // 2], b"", c.proof + b"\x00"):
        assert c.light(bad) == c.ours(bad) == -1
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        c.light(c.proof, inputs=mont_array(ins + [1]))
    assert c.light(c.proof) == 1


@pytest.mark.parametrize("s", [4, 7])
def test_nizk_wrong_statement_and_malformed_bytes(P, nizks, s):
    c = nizks(s)
    ins = from_mont_array(c.inst.inputs, c.ni)
    ins[-1] = (ins[-1] + 1) % Q
    wrong = mont_array(ins)
    assert c.light(c.proof, inputs=wrong) == c.ours(c.proof, inputs=wrong) == 0
    other = b"another_label"
    assert c.light(c.proof, label=other) == c.ours(c.proof, label=other) == c.oracle(c.proof, label=other) == 0
    for bad in (c.proof[:-1], c.proof[:len(c.proof) // 2], b"", c.proof + b"\x00"):
        assert c.light(bad) == c.ours(bad) == -1
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        c.light(c.proof, inputs=mont_array(ins + [1]))
    assert c.light(c.proof) == 1


# ---- verify_many
def mixed(c, bads, K):
    """K proofs, good and damaged in turn, ending on a truncated one when there is room"""
    pool = [c.proof, bads[0], c.oproof, bads[1], c.proof[:len(c.proof) // 2]]
    return pool[:K]


@pytest.mark.parametrize("key", [4, 7, 12])
def test_snark_verify_many(snarks, orc, key):
    c = snarks(key)
    lay = Layout(c.proof)
    bads = [flip(orc, c.proof, *lay.fields[n]) for n in ("hash_layer.proof_ops.z1", "eval_vars.L_vec")]   # leave after G_hat calls of the batch
    for K in (1, 3, 5):
        batch = mixed(c, bads, K)
        single = [c.light(p) for p in batch]
        assert single == [c.ours(p) for p in batch]
        assert c.P.SNARK.verify_many(c.ctx, c.comm, batch, c.inputs, c.vg, LABEL) == single, K
        assert c.P.SNARK.verify_many(c.ctx, c.comm, batch, c.inputs, c.gens, LABEL) == single, K
    assert single == [1, 0, 1, 0, -1]
    good = [c.proof, c.oproof, c.proof]
    assert c.P.SNARK.verify_many(c.ctx, c.comm, good, c.inputs, c.vg, LABEL) == [1, 1, 1]


@pytest.mark.parametrize("s", [4, 7, 12])
def test_nizk_verify_many(nizks, orc, s):
    c = nizks(s)
    f = field_offsets(c.proof)
    bads = [flip(orc, c.proof, f["log.z1"], "scalar"), flip(orc, c.proof, f["bullet.L_vec"], "point")]
    for K in (1, 3, 5):
        batch = mixed(c, bads, K)
        single = [c.light(p) for p in batch]
        assert single == [c.ours(p) for p in batch]
        assert c.P.NIZK.verify_many(c.ctx, c.inst, batch, c.inst.inputs, c.vg, NIZK_LABEL) == single, K
    assert single == [1, 0, 1, 0, -1]


# ---- caller-owned transcript
def test_snark_verify_t_leaves_the_transcript_where_the_prover_generators_leave_it(snarks):
    from tests.test_gpu_proofs import _caller_transcript_state
    c = snarks(7)
    st_p, st_full, st_light = (_caller_transcript_state(c.P.H, "spz_merlin_state") for _ in range(3))
    proof = c.P.SNARK.prove_t(c.ctx, c.inst, c.enc, c.vars, c.inputs, c.gens, st_p, c.tape)
    before = bytes(st_light)
    assert c.P.SNARK.verify_t(c.ctx, c.comm, proof, c.inputs, c.gens, st_full) == 1
    assert c.P.SNARK.verify_t(c.ctx, c.comm, proof, c.inputs, c.vg, st_light) == 1
    assert bytes(st_light) == bytes(st_full) == bytes(st_p) and bytes(st_light) != before


def test_nizk_verify_t_leaves_the_transcript_where_the_prover_generators_leave_it(nizks):
    from tests.test_gpu_proofs import _caller_transcript_state
    c = nizks(7)
    st_p, st_full, st_light = (_caller_transcript_state(c.P.H, "spz_merlin_state") for _ in range(3))
    proof = c.P.NIZK.prove_t(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.gens, st_p, c.tape)
    before = bytes(st_light)
    assert c.P.NIZK.verify_t(c.ctx, c.inst, proof, c.inst.inputs, c.gens, st_full) == 1
    assert c.P.NIZK.verify_t(c.ctx, c.inst, proof, c.inst.inputs, c.vg, st_light) == 1
    assert bytes(st_light) == bytes(st_full) == bytes(st_p) and bytes(st_light) != before


# ---- refusals: everything that needs the prover's window tables says so, before any device call, and the context goes on verifying
def test_snark_prover_entries_refuse_verifier_only_generators(P, snarks):
    c = snarks(4)
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.SNARK.encode(c.ctx, c.inst, c.vg)
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.SNARK.prove(c.ctx, c.inst, c.enc, c.vars, c.inputs, c.vg, LABEL, c.tape)
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.SNARK.prove(c.ctx, c.inst, c.enc, P.VarsAssignment(c.ctx, c.vars), c.inputs, c.vg, LABEL, c.tape)
    from tests.test_gpu_proofs import _caller_transcript_state
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.SNARK.prove_t(c.ctx, c.inst, c.enc, c.vars, c.inputs, c.vg, _caller_transcript_state(P.H, "spz_merlin_state"), c.tape)
    for accessor in (c.vg.window_bits, c.vg.windows, c.vg.table_bytes):
        with pytest.raises(P.SpartanHipError, match="verifier-only"):
            accessor(0)
    assert c.gens.windows(0) >= 17 and c.gens.table_bytes(1) > 0       # the prover's generators still answer
    assert c.light(c.proof) == 1 and c.ours(c.proof) == 1
    assert c.prove(c.vars, c.tape) == c.proof


def test_nizk_prover_entries_refuse_verifier_only_generators(P, nizks):
    c = nizks(4)
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.NIZK.prove(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.vg, NIZK_LABEL, c.tape)
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.NIZK.prove(c.ctx, c.inst, P.VarsAssignment(c.ctx, c.inst.vars), c.inst.inputs, c.vg, NIZK_LABEL, c.tape)
    from tests.test_gpu_proofs import _caller_transcript_state
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.NIZK.prove_t(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.vg, _caller_transcript_state(P.H, "spz_merlin_state"), c.tape)
    assert c.light(c.proof) == 1 and c.ours(c.proof) == 1
    assert c.P.NIZK.prove(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.gens, NIZK_LABEL, c.tape) == c.proof
