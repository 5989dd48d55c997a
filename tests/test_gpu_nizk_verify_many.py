"""NIZK::verify_many (spartan_amd/host/verifier.cc): K proofs of one instance verified in lock step — one host thread a proof through the
NIZK::verify body, meeting at the device calls (spartan_amd/host/batch_gate.hpp): sp_msm_var_many for C_LZ, one sp_commit_rows of K rows for
G_hat, and ONE sp_sparse_evaluate_many_begin for R1CSInstance::evaluate at the K proofs' own points, a job that belongs to the batch. Every
proof must get the verdict NIZK.verify_status gives it alone, which is the oracle's: mixed batches whose members leave the lock step at its
start, between the device calls and at its end, permutations, the batch edges (K = 0, 1, 65), all-rejected and all-malformed batches, the
trip and launch counts, and the state the context is left in."""
import ctypes, random
import pytest
from tests.helpers import *
from tests.test_gpu_verify import Case, FLIPPED, flip, field_offsets, LABEL

pytestmark = pytest.mark.gpu
SIZES = [1, 4, 10]
# one flipped bit that makes the rejection fall in the first sum-check (before any blocking device call; the evaluation is already posted),
# in the last check of the PolyEvalProof (after C_LZ and G_hat, before the evaluation is collected: that member never collects) and in the
# last equality proof (after the collect)
LEAVES_EARLY, LEAVES_MIDWAY, LEAVES_LAST = "sc1.comm_polys", "log.z1", "eq2.z"
assert {LEAVES_EARLY, LEAVES_MIDWAY, LEAVES_LAST, "rx", "ry.last"} <= set(FLIPPED)


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
    def get(s):
        if s not in made:
            made[s] = Case(P, ctx, orc, s, seed=s)
        return made[s]
    yield get
    for c in made.values():
        for oi in getattr(c, "other_oracles", []):
            orc.orc_instance_free(oi)
        c.free()


def many(c, proofs, inputs=None):
    return c.P.NIZK.verify_many(c.ctx, c.inst, proofs, c.inst.inputs if inputs is None else inputs, c.gens, LABEL)


def oracle_with_inputs(c, orc, inputs):
    """the oracle's instance once more with other public inputs (its verifier takes the inputs from the instance)"""
    nnz = [orc.orc_instance_nnz(c.oi, ctypes.c_int(k)) for k in range(3)]
    n = sum(nnz)
    rows, cols, vals = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * (4 * n))()
    vars_, ins = (ctypes.c_uint64 * (4 * c.N))(), (ctypes.c_uint64 * (4 * c.ni))()
    orc.orc_instance_export(c.oi, rows, cols, vals, vars_, ins)
    assert bytes(ins) == bytes(c.inst.inputs)[:32 * c.ni]
    oi = vp(orc.orc_instance_new(sz(c.N), sz(c.N), sz(c.ni), (sz * 3)(*nnz), rows, cols, vals, vars_, sz(c.N), inputs))
    c.other_oracles = getattr(c, "other_oracles", []) + [oi]
    return oi


_BATCH = {}


def mixed_batch(c, orc):
    """[(what, proof bytes, inputs, the oracle's verdict or None where it cannot be asked)] — built once per case, the oracle asked first"""
    if c.s in _BATCH:
        return _BATCH[c.s]
    from tests.test_oracle_pins import RFC_BAD
    offs = field_offsets(c.proof)
    flipped = lambda name: flip(orc, c.proof, name, offs[name])
    own = c.inst.inputs
    ins = from_mont_array(own, c.ni)
    ins[0] = (ins[0] + 1) % Q
    other_inputs = mont_array(ins)
    other_oi = oracle_with_inputs(c, orc, other_inputs)
    o = offs["comm_vars.last"]
    undecodable = c.proof[:o] + bytes.fromhex(RFC_BAD[6]) + c.proof[o + 32:]
    fresh = [c.P.NIZK.prove(c.ctx, c.inst, c.inst.vars, own, c.gens, LABEL, c.P.seed_scalar(b"tape", 5000 + i)) for i in range(3)]
    assert len({c.proof, *fresh}) == 4                                  # different tapes, different proofs
    members = [
        ("hip", c.proof, own),
        ("hip, another tape", fresh[0], own),
        ("flipped: " + LEAVES_EARLY, flipped(LEAVES_EARLY), own),
        ("oracle", c.oproof, own),
        ("flipped: " + LEAVES_MIDWAY, flipped(LEAVES_MIDWAY), own),
        ("flipped: rx", flipped("rx"), own),
        ("undecodable share in comm_vars", undecodable, own),
        ("truncated", c.proof[:len(c.proof) // 2], own),
        ("flipped: " + LEAVES_LAST, flipped(LEAVES_LAST), own),
        ("flipped: ry.last", flipped("ry.last"), own),
        ("hip, another proof's altered inputs", fresh[1], other_inputs),
        ("hip, a third tape", fresh[2], own),
    ]
    b = []
    for what, p, i in members:
        if what.startswith("undecodable"):     # the oracle restates the reference's decompress().unwrap() as an abort: not asked
            verdict = None
        elif i is other_inputs:
            verdict = orc.orc_nizk_verify_bytes(bytes(p), sz(len(p)), other_oi, c.og, c.digest, sz(len(c.digest)), LABEL)
        else:
            verdict = c.oracle(p)
        b.append((what, p, i, verdict))
    _BATCH[c.s] = b
    return b


EXPECT = [1, 1, 0, 1, 0, 0, None, -1, 0, 0, 0, 1]


@pytest.mark.parametrize("s", SIZES)
def test_a_mixed_batch_gets_the_single_proof_verdicts_which_are_the_oracles(cases, orc, s):
    c = cases(s)
    b = mixed_batch(c, orc)
    assert [v for *_, v in b] == EXPECT, [(w, v) for w, _, _, v in b]     # the oracle accepts every valid member and none of the others
    single = [c.ours(p, inputs=i) for _, p, i, _ in b]
    assert single == [0 if e is None else e for e in EXPECT]
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


@pytest.mark.parametrize("s", SIZES)
def test_only_the_evaluation_at_its_own_point_rejects_a_changed_point(cases, orc, s):
    """a proof whose claimed rx or ry differs in one bit passes every check but the last two (the evaluation of the instance at the CLAIMED
    point enters the last equality; the claimed point is compared at the very end): inside a batch of valid proofs it must be evaluated at its
    own point, not at a neighbour's, and the neighbours at theirs"""
    c = cases(s)
    by_name = {w: p for w, p, _, _ in mixed_batch(c, orc)}
    for name in ("flipped: rx", "flipped: ry.last"):
        assert many(c, [c.proof, by_name[name], c.oproof]) == [1, 0, 1]
        assert many(c, [by_name[name], c.proof]) == [0, 1]
        assert many(c, [by_name[name]] * 3) == [0, 0, 0]


@pytest.mark.parametrize("s", SIZES)
def test_the_flipped_members_leave_the_lock_step_where_their_names_say(cases, orc, s):
    """counted as the round trips of a batch of that proof alone, so that a change of the proof's layout or of the verifier's order cannot
    quietly move the departures: none before the first blocking call; C_LZ and G_hat before the last check of the PolyEvalProof, which comes
    before the evaluation is collected (collecting costs no trip of its own: the job is waited for on its event)"""
    from spartan_amd import capi
    c = cases(s)
    raw = c.ctx.raw()
    by_name = {w: p for w, p, _, _ in mixed_batch(c, orc)}
    for name, trips in ((LEAVES_EARLY, 0), (LEAVES_MIDWAY, 2), (LEAVES_LAST, 2)):
        t0 = capi.lib.sp_ctx_trips(raw)
        assert many(c, [by_name["flipped: " + name]]) == [0]
        assert capi.lib.sp_ctx_trips(raw) - t0 == trips, (name, trips)
    t0 = capi.lib.sp_ctx_trips(raw)                                     # and the three between valid proofs still make one batch's trips
    assert many(c, [c.proof, by_name["flipped: " + LEAVES_EARLY], by_name["flipped: " + LEAVES_MIDWAY], c.oproof, by_name["flipped: " + LEAVES_LAST]]) == [1, 0, 0, 1, 0]
    assert capi.lib.sp_ctx_trips(raw) - t0 == 2


def test_batch_edges_equal_the_single_proof_verdicts(cases, orc):
    c = cases(4)
    b = mixed_batch(c, orc)
    raw = c.ctx.raw()
    from spartan_amd import capi
    trips = lambda: capi.lib.sp_ctx_trips(raw)
    shared = [(p, c.ours(p)) for _, p, i, _ in b if i is c.inst.inputs]  # members under the instance's own inputs
    assert many(c, []) == []                                            # K = 0 is legal and does nothing
    for p, v in shared:                                                 # K = 1
        assert many(c, [p]) == [v]
    rejected = [p for p, v in shared if v == 0]
    assert len(rejected) >= 5 and many(c, rejected) == [0] * len(rejected)      # nobody collects: the caller's thread waits for the job
    malformed = [c.proof[:-1], c.proof[:7], b"", c.proof + b"\x00"]
    t0 = trips()
    assert many(c, malformed) == [-1] * 4
    assert trips() == t0                                                # malformed proofs never reach the device
    sixty_five = [shared[k % len(shared)] for k in range(65)]           # crosses the cut at 64
    assert many(c, [p for p, _ in sixty_five]) == [v for _, v in sixty_five]
    assert many(c, [c.proof] * 65) == [1] * 65


def test_wrong_number_of_inputs_is_the_callers_error(P, cases):
    c = cases(4)
    ins = from_mont_array(c.inst.inputs, c.ni)
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        many(c, [c.proof, c.proof], mont_array(ins + [1]))
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        many(c, [c.proof, c.proof], [c.inst.inputs, mont_array(ins + [1])])
    # the C entry point: -2, the error text, and no verdict
    H = P.H
    K = 2
    keep = [ctypes.create_string_buffer(c.proof, len(c.proof)) for _ in range(K)]
    pa = (vp * K)(*[ctypes.cast(x, vp) for x in keep]); la = (sz * K)(*[len(c.proof)] * K)
    wrong = mont_array(ins + [1])
    ia = (vp * K)(*[ctypes.cast(wrong, vp)] * K)
    st = (ctypes.c_int * K)(1, 1)
    rc = H.spz_nizk_verify_many(c.ctx.h, c.inst.h, c.gens.h, pa, la, ia, sz(len(wrong) // 4), sz(K), LABEL, st)
    assert rc == -2 and b"InvalidNumberOfInputs" in H.spz_last_error() and 1 not in list(st)
    assert H.spz_nizk_verify_many(c.ctx.h, c.inst.h, c.gens.h, None, None, None, sz(0), sz(0), LABEL, None) == 0
    assert H.spz_nizk_verify_many(c.ctx.h, c.inst.h, c.gens.h, None, la, ia, sz(c.ni), sz(K), LABEL, st) == -2
    assert many(c, [c.proof]) == [1]


def _counted(c, fn):
    """(result, round trips, launches per family) of fn() on the case's context"""
    from spartan_amd import capi
    L, raw = capi.lib, c.ctx.raw()
    assert L.sp_prof_enable(raw, ctypes.c_int(1)) == 0 and L.sp_prof_reset(raw) == 0
    t0 = L.sp_ctx_trips(raw)
    got = fn()
    trips = L.sp_ctx_trips(raw) - t0
    cap = 64
    names = (ctypes.c_char_p * cap)(); ms = (ctypes.c_double * cap)(); n = (ctypes.c_uint64 * cap)(); by = (ctypes.c_double * cap)()
    k = L.sp_prof_read(raw, names, ms, n, by, ctypes.c_int(cap))
    L.sp_prof_enable(raw, ctypes.c_int(0))
    return got, trips, {names[i].decode(): int(n[i]) for i in range(k)}


def test_placement_of_a_batch_at_2_10(cases):
    """a batch of up to 64 proofs makes the round trips of ONE verification, one C_LZ launch chain, and no more launches of the sparse and
    eq_expand families than one verification — whatever K is: the evaluation is one record of `sparse` and builds no table through sp_eq_expand"""
    c = cases(10)
    proofs = [c.proof, c.oproof] + [c.P.NIZK.prove(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.gens, LABEL, c.P.seed_scalar(b"tape", 7000 + i)) for i in range(14)]
    assert many(c, proofs[:2]) == [1, 1] and c.ours(c.proof) == 1       # warm: the digest and the host-side generator tables exist
    one, one_trips, one_fam = _counted(c, lambda: c.ours(c.proof))
    assert one == 1 and one_fam["msm_var"] == 1 and one_fam["sparse"] >= 1
    for K in (1, 2, 16):
        got, trips, fam = _counted(c, lambda: many(c, proofs[:K]))
        print("round trips per NIZK::verify_many of %d proofs at 2^10:" % K, trips, "(one verify: %d)" % one_trips, "launches:", {a: b for a, b in fam.items() if b})
        assert got == [1] * K
        assert trips <= one_trips, (K, trips, one_trips)
        assert fam["msm_var"] == 1, (K, fam)
        assert fam["sparse"] <= one_fam["sparse"] and fam["eq_expand"] <= one_fam["eq_expand"], (K, fam, one_fam)
        assert fam["sparse"] == 1


def test_the_context_is_left_as_it_was(cases, orc):
    c = cases(4)
    b = mixed_batch(c, orc)
    many(c, [p for _, p, _, _ in b], [i for _, _, i, _ in b])
    assert c.ours(c.proof) == 1
    assert c.P.NIZK.verify(c.ctx, c.inst, c.proof, c.inst.inputs, c.gens, LABEL) is True
    again = c.P.NIZK.prove(c.ctx, c.inst, c.inst.vars, c.inst.inputs, c.gens, LABEL, c.tape)
    assert again == c.proof                                             # a new proof, byte for byte the one from before the batches
