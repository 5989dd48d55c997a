"""SNARK::verify_many (spartan_amd/host/verifier.cc): K proofs of one circuit verified in lock step — one host thread a proof through the
unchanged SNARK::verify, meeting at the device calls (spartan_amd/host/batch_gate.hpp), which go out as sp_msm_var_many,
sp_msm_points_many and one sp_commit_rows of K rows. Every proof must get the verdict SNARK.verify_status gives it alone, which is the
oracle's: mixed batches whose members leave the lock step at its start, in its middle and at its end, permutations, the batch edges
(K = 0, 1, 65), all-rejected and all-malformed batches, the trip count, and the state the context is left in."""
import ctypes, random
import pytest
from tests.helpers import *
from tests import structured_cases as sc
from tests.snark_layout import Layout
from tests.test_gpu_snark_verify import Case, FLIPPED, flip

pytestmark = pytest.mark.gpu
LABEL = sc.SNARK_LABEL
KEYS = [4, 10, "shifted"]
# one flipped bit that makes the rejection fall in the first sum-check of r1cs_sat_proof (before any device call), in its PolyEvalProof (after
# the first C_LZ and G_hat) and in the PolyEvalProof that r1cs_eval_proof verifies last (proof_mem: after all eight)
LEAVES_EARLY, LEAVES_MIDWAY, LEAVES_LAST = "sc1.comm_polys", "eval_vars.z1", "hash_layer.proof_mem.z2"
assert {LEAVES_EARLY, LEAVES_MIDWAY, LEAVES_LAST} <= set(FLIPPED)


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


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


def many(c, proofs, inputs=None):
    return c.P.SNARK.verify_many(c.ctx, c.comm, proofs, c.inputs if inputs is None else inputs, c.gens, LABEL)


_BATCH = {}


def mixed_batch(c, orc):
    """[(what, proof bytes, inputs, ask the oracle)] — built once per case"""
    if c.key in _BATCH:
        return _BATCH[c.key]
    from tests.test_oracle_pins import RFC_BAD
    lay = Layout(c.proof)
    flipped = lambda name: flip(orc, c.proof, *lay.fields[name])
    ins = from_mont_array(c.inputs, c.n_inputs)
    ins[0] = (ins[0] + 1) % Q
    other_inputs = mont_array(ins)
    o = lay.fields["comm_vars.last"][0]
    undecodable = c.proof[:o] + bytes.fromhex(RFC_BAD[6]) + c.proof[o + 32:]
    fresh = [c.prove(c.vars, c.P.seed_scalar(b"tape", 5000 + i)) for i in range(3)]
    assert len({c.proof, *fresh}) == 4                                  # different tapes, different proofs
    b = [
        ("hip", c.proof, c.inputs, True),
        ("hip, another tape", fresh[0], c.inputs, True),
        ("flipped: " + LEAVES_EARLY, flipped(LEAVES_EARLY), c.inputs, True),
        ("oracle", c.oproof, c.inputs, True),
        ("flipped: " + LEAVES_MIDWAY, flipped(LEAVES_MIDWAY), c.inputs, True),
        # the oracle restates the reference's decompress().unwrap() as an abort: it is not asked about a point that does not decode
        ("undecodable share in comm_vars", undecodable, c.inputs, False),
        ("truncated", c.proof[:len(c.proof) // 2], c.inputs, True),
        ("flipped: " + LEAVES_LAST, flipped(LEAVES_LAST), c.inputs, True),
        ("hip, another proof's altered inputs", fresh[1], other_inputs, True),
        ("hip, a third tape", fresh[2], c.inputs, True),
    ]
    _BATCH[c.key] = b
    return b


@pytest.mark.parametrize("key", KEYS)
def test_a_mixed_batch_gets_the_single_proof_verdicts_which_are_the_oracles(cases, orc, key):
    c = cases(key)
    b = mixed_batch(c, orc)
    # the oracle alone, on the CPU, first: it accepts every valid member and none of the others
    oracle = [c.oracle(p, inputs=i) if ask else None for _, p, i, ask in b]
    expect = [1, 1, 0, 1, 0, None, -1, 0, 0, 1]
    assert oracle == expect, list(zip([w for w, *_ in b], oracle))
    single = [c.ours(p, inputs=i) for _, p, i, _ in b]
    assert single == [0 if e is None else e for e in expect]
    assert {1, 0, -1} <= set(single)                                   # a member of each verdict
    got = many(c, [p for _, p, _, _ in b], [i for _, _, i, _ in b])
    assert got == single, list(zip([w for w, *_ in b], got, single))
    # the same batch permuted gives the permuted verdicts
    order = list(range(len(b)))
    for seed in (1, 2):
        random.Random(seed).shuffle(order)
        got = many(c, [b[i][1] for i in order], [b[i][2] for i in order])
        assert got == [single[i] for i in order], order
    got = many(c, [b[i][1] for i in reversed(range(len(b)))], [b[i][2] for i in reversed(range(len(b)))])
    assert got == single[::-1]


@pytest.mark.parametrize("key", KEYS)
def test_the_flipped_members_leave_the_lock_step_where_their_names_say(cases, orc, key):
    """the three flipped fields are chosen so that a member leaves before the first device call, after the first PolyEvalProof's two and
    after all eight: counted as the round trips of a batch of that proof alone, so that a change of the proof's layout or of the
    verifier's order cannot quietly move all three departures to one place"""
    from spartan_amd import capi
    c = cases(key)
    raw = c.ctx.raw()
    by_name = {w: p for w, p, _, _ in mixed_batch(c, orc)}
    for name, trips in ((LEAVES_EARLY, 0), (LEAVES_MIDWAY, 2), (LEAVES_LAST, 8)):
        t0 = capi.lib.sp_ctx_trips(raw)
        assert many(c, [by_name["flipped: " + name]]) == [0]
        assert capi.lib.sp_ctx_trips(raw) - t0 == trips, (name, trips)
    t0 = capi.lib.sp_ctx_trips(raw)                                     # and the three between valid proofs still make one batch's trips
    assert many(c, [c.proof, by_name["flipped: " + LEAVES_EARLY], by_name["flipped: " + LEAVES_MIDWAY], c.oproof, by_name["flipped: " + LEAVES_LAST]]) == [1, 0, 0, 1, 0]
    assert capi.lib.sp_ctx_trips(raw) - t0 == 8


def test_batch_edges_equal_the_single_proof_verdicts(cases, orc):
    c = cases(4)
    b = mixed_batch(c, orc)
    raw = c.ctx.raw()
    from spartan_amd import capi
    trips = lambda: capi.lib.sp_ctx_trips(raw)
    shared = [(p, c.ours(p)) for _, p, i, _ in b if i is c.inputs]      # members under the shared inputs buffer
    assert many(c, []) == []                                            # K = 0 is legal and does nothing
    for p, v in shared:                                                 # K = 1
        assert many(c, [p]) == [v]
    rejected = [p for p, v in shared if v == 0]
    assert len(rejected) >= 4 and many(c, rejected) == [0] * len(rejected)
    malformed = [c.proof[:-1], c.proof[:7], b"", c.proof + b"\x00"]
    t0 = trips()
    assert many(c, malformed) == [-1] * 4
    assert trips() == t0                                                # malformed proofs never reach the device
    sixty_five = [shared[k % len(shared)] for k in range(65)]           # crosses the cut at 64
    assert many(c, [p for p, _ in sixty_five]) == [v for _, v in sixty_five]
    assert many(c, [c.proof] * 65) == [1] * 65


def test_wrong_number_of_inputs_is_the_callers_error(P, cases):
    c = cases(4)
    ins = from_mont_array(c.inputs, c.n_inputs)
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        many(c, [c.proof, c.proof], mont_array(ins + [1]))
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        many(c, [c.proof, c.proof], [c.inputs, mont_array(ins + [1])])
    # the C entry point: -2, the error text, and no verdict
    H = P.H
    K = 2
    keep = [ctypes.create_string_buffer(c.proof, len(c.proof)) for _ in range(K)]
    pa = (vp * K)(*[ctypes.cast(x, vp) for x in keep]); la = (sz * K)(*[len(c.proof)] * K)
    short = mont_array(ins[:-1]) if len(ins) > 1 else mont_array(ins + [1])
    ia = (vp * K)(*[ctypes.cast(short, vp)] * K)
    st = (ctypes.c_int * K)(1, 1)
    rc = H.spz_snark_verify_many(c.ctx.h, c.comm.h, c.gens.h, pa, la, ia, sz(len(short) // 4), sz(K), LABEL, st)
    assert rc == -2 and b"InvalidNumberOfInputs" in H.spz_last_error() and 1 not in list(st)
    assert H.spz_snark_verify_many(c.ctx.h, c.comm.h, c.gens.h, None, None, None, sz(0), sz(0), LABEL, None) == 0
    assert H.spz_snark_verify_many(c.ctx.h, c.comm.h, c.gens.h, None, la, ia, sz(c.n_inputs), sz(K), LABEL, st) == -2
    assert many(c, [c.proof]) == [1]


def test_placement_of_a_batch_at_2_10(cases):
    """a batch of up to 64 proofs makes the round trips of ONE verification: 4 C_LZ (2 sp_msm_var_many, 2 sp_msm_points_many) and 4 G_hat
    (sp_commit_rows with one row a proof) — the count test_placement_of_a_verification_at_2_10 derives for a single proof"""
    from spartan_amd import capi
    c = cases(10)
    raw = c.ctx.raw()
    L = capi.lib
    proofs = [c.proof, c.oproof] + [c.prove(c.vars, c.P.seed_scalar(b"tape", 7000 + i)) for i in range(14)]
    assert many(c, proofs[:2]) == [1, 1]                              # warm: the host-side generator tables exist
    for K in (1, 2, 16):
        assert L.sp_prof_enable(raw, ctypes.c_int(1)) == 0 and L.sp_prof_reset(raw) == 0
        t0 = L.sp_ctx_trips(raw)
        got = many(c, proofs[:K])
        trips = L.sp_ctx_trips(raw) - t0
        cap = 64
        names = (ctypes.c_char_p * cap)(); ms = (ctypes.c_double * cap)(); n = (ctypes.c_uint64 * cap)(); by = (ctypes.c_double * cap)()
        k = L.sp_prof_read(raw, names, ms, n, by, ctypes.c_int(cap))
        L.sp_prof_enable(raw, ctypes.c_int(0))
        fam = {names[i].decode(): int(n[i]) for i in range(k)}
        print("round trips per SNARK::verify_many of %d proofs at 2^10:" % K, trips, "launches:", {a: b for a, b in fam.items() if b})
        assert got == [1] * K
        assert trips <= 8, (K, trips)
        assert fam["msm_var"] == 2 and fam["msm_points"] == 2, (K, fam)


def test_the_context_is_left_as_it_was(cases, orc):
    c = cases(4)
    b = mixed_batch(c, orc)
    many(c, [p for _, p, _, _ in b], [i for _, _, i, _ in b])
    assert c.ours(c.proof) == 1
    assert c.prove(c.vars, c.tape) == c.proof                           # a new proof, byte for byte the one from before the batches
