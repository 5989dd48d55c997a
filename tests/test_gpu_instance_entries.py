"""Instance.from_entries and Instance.from_tensors (spartan_amd/prover.py over Instance::from_entries / from_device_entries and
sp_sparse_from_entries) next to Instance.new on the structured cases of tests/structured_cases.py: the same digest, the same satisfiability
report, the same SNARK::encode commitment and the same SNARK and NIZK proof bytes under the case's tape seed — the bytes the structured tests
pin to the oracle — and the proofs verify. Then the instances of 0 and 1 constraints (the pad entries), the precedence of the two errors
across matrices, and the context after a refusal."""
import ctypes
import pytest
from tests.helpers import *
from tests import sparse_build_reference as sb
from tests import structured_cases as sc

pytestmark = pytest.mark.gpu
SMALL = list(sc.SMALL)
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


def _pack(A, B, C):
    ent = list(A) + list(B) + list(C)
    n = max(len(ent), 1)
    return ([len(A), len(B), len(C)], (u64 * n)(*[e[0] for e in ent]), (u64 * n)(*[e[1] for e in ent]),
            b"".join(e[2].to_bytes(32, "little") for e in ent))


def _tensors(mats, offset=0):
    """[(rows, cols, vals)] on the GPU; rows and cols as int64 bit patterns of the unsigned values, vals `offset` bytes into a larger tensor"""
    import torch
    out = []
    for m in mats:
        n = len(m)
        signed = lambda x: x - 2**64 if x >= 2**63 else x
        r = torch.tensor([signed(e[0]) for e in m], dtype=torch.int64).cuda()
        c = torch.tensor([signed(e[1]) for e in m], dtype=torch.int64).cuda()
        big = torch.frombuffer(bytearray(bytes(offset) + b"".join(e[2].to_bytes(32, "little") for e in m) + bytes(8)), dtype=torch.uint8).cuda()
        out.append((r, c, big[offset:offset + 32 * n]))
    torch.cuda.synchronize()
    return out


def _make(P, ctx, how, nc, nv, ni, A, B, C):
    if how == "new":
        return P.Instance.new(ctx, nc, nv, ni, *_pack(A, B, C))
    if how == "entries":
        nnz, rows, cols, vals = _pack(A, B, C)
        return P.Instance.from_entries(ctx, nc, nv, ni, nnz, rows, cols, bytearray(vals))   # any buffer of 32 n bytes
    return P.Instance.from_tensors(ctx, nc, nv, ni, *_tensors((A, B, C), offset=1))


def _report(inst, vars_, inputs, max_rows=64):
    r = inst.check(vars_, inputs, max_rows=max_rows)
    return r.violated, r.first_row, r.rows


@pytest.mark.parametrize("name", SMALL)
def test_structured_cases_match_instance_new_and_the_oracle(P, ctx, orc, name):
    run = sc.oracle_run(orc, name)
    pk, case = run.pk, run.case
    nc, nv, ni, A, B, C = case[:6]
    w = list(case[6]); w[sc.BREAKING_VAR[name]] = (w[sc.BREAKING_VAR[name]] + 1) % Q
    truth = sc.failing_rows(case, vars_=w)
    broken = mont_bulk(w)
    tape = P.seed_scalar(b"tape", sc.TAPE_SEED[name])
    gens = P.SNARKGens(ctx, *run.gens_args)
    ngens = P.NIZKGens(ctx, *run.gens_args[:3])
    ref = None
    for how in ("new", "entries", "tensors"):
        inst = _make(P, ctx, how, nc, nv, ni, A, B, C)
        got = {"digest": inst.digest(), "sat": _report(inst, pk.vars, pk.inputs), "broken": _report(inst, broken, pk.inputs, len(truth))}
        inst.set_digest(run.digest)
        got["nizk"] = P.NIZK.prove(ctx, inst, pk.vars, pk.inputs, ngens, sc.NIZK_LABEL, tape)
        enc = P.SNARK.encode(ctx, inst, gens)
        got["commitment"] = enc.serialize_commitment()
        got["snark"] = P.SNARK.prove(ctx, inst, enc, pk.vars, pk.inputs, gens, sc.SNARK_LABEL, tape)
        assert got["sat"] == (0, None, []) and got["broken"] == (len(truth), truth[0], truth)
        assert got["nizk"] == run.nizk and got["commitment"] == run.commitment and got["snark"] == run.snark, how   # the oracle's bytes
        assert P.NIZK.verify_status(ctx, inst, got["nizk"], pk.inputs, ngens, sc.NIZK_LABEL) == 1
        comm = P.Commitment.encode(ctx, inst, gens)               # the verifier's commitment to the circuit itself, from the resident entries
        assert comm.serialize() == run.commitment
        assert P.SNARK.verify_status(ctx, comm, got["snark"], pk.inputs, gens, sc.SNARK_LABEL) == 1
        assert P.SNARK.verify_status(ctx, comm, got["snark"], run.wrong_inputs(), gens, sc.SNARK_LABEL) == 0
        comm.free(); enc.free(); inst.free()
        if ref is None:
            ref = got
        for key in ref:
            assert got[key] == ref[key], (how, key)
    ngens.free(); gens.free()


# lib.rs:672-753 test_padded_constraints (a^2 + b + 13 = z over inputs (16, 1, 2)): A and B have fewer entries than num_cons_padded = 2 and get
# one pad entry each, C has more and gets none
PADDED = ([(0, 2, 1)], [(0, 2, 1)], [(0, 1, 1), (0, 0, Q - 13), (0, 3, Q - 1)])


@pytest.mark.parametrize("nc,mats,proves", [
    (1, PADDED, True),
    (1, ([(0, 2, 1)], [], [(0, 0, 5), (0, 0, Q - 5)]), False),     # no entry: two pad entries; exactly num_cons_padded entries: none
    (0, ([], [], []), False),                                     # no constraint at all: num_cons_padded is 1, one pad entry per matrix
])
def test_zero_and_one_constraints(P, ctx, nc, mats, proves):
    """num_cons of 0 and 1: the reference adds explicit zero constraints (i, num_vars, 0) for i in len..num_cons_padded (lib.rs:191-195)"""
    nv, ni = 0, 3
    st, shape, built = sb.instance_new(nc, nv, ni, *mats)
    assert st == "ok" and shape == ((2 if nc else 1), 4)
    assert [len(b) - len(m) for b, m in zip(built, mats)] == [shape[0] - min(len(m), shape[0]) for m in mats]
    vars_, inputs = (u64 * 0)(), mont_bulk([16, 1, 2])
    z = [0, 0, 0, 0, 1, 16, 1, 2]
    bad_rows = sb.violated_rows(*built, z, shape[0])
    ref = None
    for how in ("new", "entries", "tensors"):
        inst = _make(P, ctx, how, nc, nv, ni, *mats)
        got = {"digest": inst.digest(), "check": _report(inst, vars_, inputs)}
        assert got["check"] == (len(bad_rows), bad_rows[0] if bad_rows else None, bad_rows)
        if proves:
            assert bad_rows == []
            inst.set_digest(b"padded")
            tape = P.seed_scalar(b"tape", 77)
            ngens = P.NIZKGens(ctx, nc, nv, ni)
            got["nizk"] = P.NIZK.prove(ctx, inst, vars_, inputs, ngens, sc.NIZK_LABEL, tape)
            assert P.NIZK.verify_status(ctx, inst, got["nizk"], inputs, ngens, sc.NIZK_LABEL) == 1
            gens = P.SNARKGens(ctx, nc, nv, ni, 3)
            enc = P.SNARK.encode(ctx, inst, gens)
            got["commitment"] = enc.serialize_commitment()
            got["snark"] = P.SNARK.prove(ctx, inst, enc, vars_, inputs, gens, sc.SNARK_LABEL, tape)
            comm = enc.commitment(ctx)
            assert P.SNARK.verify_status(ctx, comm, got["snark"], inputs, gens, sc.SNARK_LABEL) == 1
            comm.free(); enc.free(); gens.free(); ngens.free()
        inst.free()
        if ref is None:
            ref = got
        assert got == ref, how


def test_error_precedence_across_matrices_and_the_context_afterwards(P, ctx, orc):
    good = [(0, 0, 1), (1, 1, 2), (1, 2, 3)]
    cases = [
        # A with a bad scalar in its last entry, B with a bad index in its first: A is parsed to its end first
        ((good + [(1, 0, Q)], [(2, 0, 1)] + good, good), P.InvalidScalar, 0, 3, 1),
        ((good + [(1, 3, 1)], [(0, 0, Q + 1)] + good, good), P.InvalidIndex, 0, 3, 1),
        ((good, good + [(0, 0, 2**255), (0, 0, 2**256 - 1)], [(7, 7, 1)]), P.InvalidScalar, 1, 3, 2),
        ((good, [], [(0, 0, 1), (2**32, 0, 1), (0, 2**32 + 1, Q)]), P.InvalidIndex, 2, 1, 2),
        ((good, good, [(0, 0, 1), (2**64 - 1, 0, 1)]), P.InvalidIndex, 2, 1, 1),             # a negative int64 in a tensor
    ]
    for mats, exc, matrix, first, count in cases:
        want = sb.instance_new(2, 2, 0, *mats)
        assert want[:2] == (exc.__name__, matrix)
        for how in ("entries", "tensors"):
            with pytest.raises(exc) as e:
                _make(P, ctx, how, 2, 2, 0, *mats)
            assert (e.value.matrix, e.value.first, e.value.count) == (matrix, first, count), how
            assert "%s: matrix %s entry %d (%d of %d entries" % (exc.__name__, "ABC"[matrix], first, count, len(mats[matrix])) in str(e.value)
        with pytest.raises(P.SpartanHipError) as e:            # Instance.new stops at the same entry with the same error
            _make(P, ctx, "new", 2, 2, 0, *mats)
        assert exc.__name__ in str(e.value)
    # after the refusals the context still proves, and gives the oracle's bytes
    name = "c_sparse"
    run = sc.oracle_run(orc, name)
    nc, nv, ni, A, B, C = run.case[:6]
    inst = _make(P, ctx, "tensors", nc, nv, ni, A, B, C)
    inst.set_digest(run.digest)
    ngens = P.NIZKGens(ctx, *run.gens_args[:3])
    assert P.NIZK.prove(ctx, inst, run.pk.vars, run.pk.inputs, ngens, sc.NIZK_LABEL, P.seed_scalar(b"tape", sc.TAPE_SEED[name])) == run.nizk
    ngens.free(); inst.free()


def test_from_tensors_refuses_what_it_cannot_read(P, ctx):
    import torch
    (r, c, v), = _tensors(([(0, 0, 1), (1, 1, 2)],))
    empty = _tensors(([],))[0]
    ok = P.Instance.from_tensors(ctx, 2, 2, 0, (r, c, v), empty, empty)      # empty matrices are legal
    new = _make(P, ctx, "new", 2, 2, 0, [(0, 0, 1), (1, 1, 2)], [], [])
    assert ok.digest() == new.digest()
    ok.free(); new.free()
    for bad in ((r.cpu(), c, v), (r.cpu().to(torch.int32).cuda(), c, v), (r, c, v[:33]), (r, c[:1], v), (r, c)):
        with pytest.raises(P.SpartanHipError):
            P.Instance.from_tensors(ctx, 2, 2, 0, bad, empty, empty)
