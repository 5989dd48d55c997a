"""Commitment.encode (spz_commitment_encode -> SNARK::encode_commitment, spartan_amd/host/verifier.cc): the verifier computes the commitment of
the circuit it verifies against from the instance itself, under either kind of generators — under verifier-only ones through
sp_commit_rows_points over the resident point sets, without a window table. The bytes are SNARK.encode's and the oracle's; proofs verify under
the handle as under a loaded one; a circuit with one value changed gets another commitment, under which the original proof is rejected; the
dense representation is not kept."""
import ctypes
import pytest
from tests.helpers import *
from tests import structured_cases as sc
from tests.test_gpu_snark_verify import comm_header
from tests.test_gpu_verifier_gens import Snark, snark_flips, LABEL

pytestmark = pytest.mark.gpu
SYNTHETIC = [1, 2, 4, 7, 10, 12]
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


class Encoded(Snark):
    """the case of tests/test_gpu_verifier_gens.py with the handle Commitment.encode computes under its verifier-only generators"""
    def __init__(self, P, ctx, orc, key):
        super().__init__(P, ctx, orc, key)
        self.handle = P.Commitment.encode(ctx, self.inst, self.vg)

    def under(self, comm, b, gens=None):
        return self.P.SNARK.verify_status(self.ctx, comm, b, self.inputs, gens or self.vg, LABEL)

    def free(self):
        self.handle.free()
        super().free()


@pytest.fixture(scope="module")
def cases(P, ctx, orc):
    made = {}
    def get(key):
        if key not in made:
            made[key] = Encoded(P, ctx, orc, key)
        return made[key]
    yield get
    for c in made.values():
        c.free()


@pytest.mark.parametrize("key", SYNTHETIC + STRUCTURED)
def test_the_bytes_are_encodes_and_the_oracles(P, cases, orc, key):
    c = cases(key)
    light = c.handle.serialize()
    full = P.Commitment.encode(c.ctx, c.inst, c.gens)
    try:
        assert light == full.serialize() == c.enc.serialize_commitment() == sc.oracle_bytes(orc, orc.orc_commitment_bincode, c.oe)
        _, ops, mem = comm_header(light)
        shares = (len(ops) + len(mem)) // 32
        assert c.handle.resident_bytes() == full.resident_bytes() == 65536 * shares
        assert c.comm.serialize() == light and c.comm.resident_bytes() == 65536 * shares          # a loaded handle serialises too
    finally:
        full.free()


@pytest.mark.parametrize("key", SYNTHETIC + STRUCTURED)
def test_proofs_are_accepted_under_the_encoded_handle(cases, key):
    c = cases(key)
    assert c.under(c.handle, c.proof) == 1
    assert c.under(c.handle, c.oproof) == 1
    assert c.under(c.handle, c.proof, gens=c.gens) == 1


@pytest.mark.parametrize("key", [4, 7])
def test_flipped_proofs_get_the_verdict_of_a_loaded_commitment(cases, orc, key):
    c = cases(key)
    for name, bad in snark_flips(c, orc):
        got, loaded = c.under(c.handle, bad), c.light(bad)
        assert got == loaded and got != 1, (name, got, loaded)
    assert c.under(c.handle, c.proof) == 1


def test_verify_many_and_verify_t_take_the_handle(cases, orc):
    from tests.test_gpu_proofs import _caller_transcript_state
    c = cases(7)
    bad = [b for _, b in snark_flips(c, orc)][0]
    batch = [c.proof, bad, c.oproof, c.proof[:len(c.proof) // 2]]
    assert c.P.SNARK.verify_many(c.ctx, c.handle, batch, c.inputs, c.vg, LABEL) == [1, 0, 1, -1]
    assert c.P.SNARK.verify_many(c.ctx, c.handle, batch, c.inputs, c.vg, LABEL) == c.P.SNARK.verify_many(c.ctx, c.comm, batch, c.inputs, c.vg, LABEL)
    st_p, st_v = (_caller_transcript_state(c.P.H, "spz_merlin_state") for _ in range(2))
    proof = c.P.SNARK.prove_t(c.ctx, c.inst, c.enc, c.vars, c.inputs, c.gens, st_p, c.tape)
    assert c.P.SNARK.verify_t(c.ctx, c.handle, proof, c.inputs, c.vg, st_v) == 1
    assert bytes(st_v) == bytes(st_p)


@pytest.mark.parametrize("name", STRUCTURED)
def test_a_substituted_circuit_gets_another_commitment(P, cases, name):
    """the same instance with one value of A changed: the verifier that encodes it itself notices what a verifier handed bytes could not"""
    c = cases(name)
    num_cons, num_vars, num_inputs, A, B, C, v, i = sc.get(name)
    A2 = list(A)
    row, col, val = A2[0]
    A2[0] = (row, col, (val + 1) % Q)
    pk = sc.Packed((num_cons, num_vars, num_inputs, A2, B, C, v, i))
    inst2 = P.Instance.new(c.ctx, pk.num_cons, pk.num_vars, pk.num_inputs, pk.nnz, pk.rows, pk.cols, pk.vals)
    other = P.Commitment.encode(c.ctx, inst2, c.vg)
    try:
        assert other.serialize() != c.handle.serialize() and len(other.serialize()) == len(c.handle.serialize())
        assert c.under(other, c.proof) == 0
        assert c.under(c.handle, c.proof) == 1
    finally:
        other.free(); inst2.free()


def test_snark_encode_still_refuses_and_the_context_goes_on(P, cases):
    c = cases(4)
    with pytest.raises(P.SpartanHipError, match="verifier-only"):
        P.SNARK.encode(c.ctx, c.inst, c.vg)
    h = P.Commitment.encode(c.ctx, c.inst, c.vg)
    try:
        assert c.prove(c.vars, c.tape) == c.proof
        assert c.under(h, c.proof) == 1 and c.ours(c.proof) == 1 and c.light(c.proof) == 1
    finally:
        h.free()


def test_encode_cycles_do_not_keep_the_dense_tables(P, cases):
    import torch
    c = cases(10)
    table_bytes = 32 * 16 * (1 << 10)        # comb_ops at 2^10: 15 polynomials of 2^10 entries padded to 16
    free_after = []
    for k in range(20):
        h = P.Commitment.encode(c.ctx, c.inst, c.vg)
        assert h.serialize() == c.comm_bytes
        h.free()
        torch.cuda.synchronize()
        free_after.append(torch.cuda.mem_get_info(0)[0])
    assert abs(free_after[-1] - free_after[1]) <= table_bytes, free_after
