"""Instance::is_sat on the device (sp_r1cs_check behind spartan_amd.prover.Instance.is_sat / .check): the verdict, the number of violated
constraints, the first one and the list of failing rows against the oracle's R1CSShape::is_sat and Python big-int arithmetic over the
instance's exported entries. Every comparison is exact."""
import ctypes, random
import pytest
from tests.helpers import *
from tests.structured_cases import _skewed_instance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


def _trips(ctx):
    from spartan_amd import capi
    return int(capi.lib.sp_ctx_trips(ctx.raw()))


def _export(orc, oi, num_vars, num_inputs):
    """entries of the oracle instance as (nnz[3], rows, cols, Montgomery vals) plus its assignment"""
    nnz = [orc.orc_instance_nnz(oi, ctypes.c_int(k)) for k in range(3)]
    tot = sum(nnz)
    rows = (ctypes.c_uint64 * tot)(); cols = (ctypes.c_uint64 * tot)(); vals = (ctypes.c_uint64 * (4 * tot))()
    vars_ = (ctypes.c_uint64 * (4 * num_vars))(); inputs = (ctypes.c_uint64 * (4 * max(num_inputs, 1)))()
    orc.orc_instance_export(oi, rows, cols, vals, vars_, inputs)
    return nnz, rows, cols, vals, vars_, inputs


def _failing_rows(nnz, rows, cols, vals_int, z, num_cons):
    """{r : (A z)[r] * (B z)[r] != (C z)[r]} by big-int arithmetic; every entry adds (duplicates included), a row without entries is satisfied"""
    acc = [[0] * num_cons for _ in range(3)]
    off = 0
    for k in range(3):
        a = acc[k]
        for i in range(off, off + nnz[k]):
            a[rows[i]] += vals_int[i] * z[cols[i]]
        off += nnz[k]
    return [r for r in range(num_cons) if (acc[0][r] % Q) * (acc[1][r] % Q) % Q != acc[2][r] % Q]


def _z(vars_int, inputs_int, num_vars_padded):
    z = list(vars_int) + [0] * (num_vars_padded - len(vars_int)) + [1] + list(inputs_int)
    return z + [0] * (2 * num_vars_padded - len(z))


def _check_report(rep, truth, max_rows):
    assert rep.violated == len(truth)
    assert rep.first_row == (truth[0] if truth else None)
    assert rep.rows == truth[:max_rows]
    assert bool(rep) == (not truth)


@pytest.mark.parametrize("s", [10, 16, 20])
def test_satisfied_synthetic_instances(P, ctx, orc, s):
    N = 1 << s
    orc.orc_set_threads(ctypes.c_int(16 if s >= 16 else 1))
    inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, 10, seed=s)
    t0 = _trips(ctx)
    assert inst.is_sat(inst.vars, inst.inputs) is True
    assert _trips(ctx) == t0 + 1
    rep = inst.check(inst.vars, inst.inputs, max_rows=8)
    assert rep.violated == 0 and rep.first_row is None and rep.rows == []
    va = P.VarsAssignment(ctx, inst.vars)
    t0 = _trips(ctx)
    assert inst.is_sat(va, inst.inputs) is True
    assert _trips(ctx) == t0 + 1
    rep = inst.check(va, inst.inputs)
    assert rep.violated == 0 and rep.first_row is None and rep.rows == []
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(10), ctypes.c_uint64(s)))
    assert orc.orc_instance_is_sat(oi) == 1
    orc.orc_instance_free(oi); va.free(); inst.free()


@pytest.mark.parametrize("s", [10, 16])
def test_wrong_witness_exact_report(P, ctx, orc, s):
    N, ni, seed = 1 << s, 10, 40 + s
    orc.orc_set_threads(ctypes.c_int(16 if s >= 16 else 1))
    inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
    nnz, rows, cols, vals, ovars, oinputs = _export(orc, oi, N, ni)
    assert list(ovars) == list(inst.vars) and list(oinputs)[:4 * ni] == list(inst.inputs)[:4 * ni]
    vals_int = from_mont_bulk(vals, sum(nnz))
    rows, cols = list(rows), list(cols)
    good_vars, good_inputs = from_mont_bulk(inst.vars, N), from_mont_bulk(inst.inputs, ni)
    assert _failing_rows(nnz, rows, cols, vals_int, _z(good_vars, good_inputs, N), N) == []
    rng = random.Random(seed)
    cases = [("interior variable", {N // 3: rng.randrange(Q)}, {}),
             ("last variable", {N - 1: rng.randrange(Q)}, {}),
             ("one input", {}, {0: rng.randrange(Q)}),         # the synthetic constraints read z up to index num_vars + 2: inputs 0 and 1
             ("100 variables", {j: rng.randrange(Q) for j in rng.sample(range(N), 100)}, {})]
    for k, (name, dv, di) in enumerate(cases):
        v, i = list(good_vars), list(good_inputs)
        for j, x in dv.items():
            v[j] = x
        for j, x in di.items():
            i[j] = x
        truth = _failing_rows(nnz, rows, cols, vals_int, _z(v, i, N), N)
        assert truth, name
        bv, bi = mont_bulk(v), mont_bulk(i)
        src = P.VarsAssignment(ctx, bv) if k % 2 else bv     # host limbs and a resident assignment in turn
        assert inst.is_sat(src, bi) is False, name
        t0 = _trips(ctx)
        rep = inst.check(src, bi, max_rows=N)
        assert _trips(ctx) == t0 + 2, name                    # the verdict, then the bitmap
        _check_report(rep, truth, N)
        few = max(1, len(truth) // 2)
        _check_report(inst.check(src, bi, max_rows=few), truth, few)
        _check_report(inst.check(src, bi, max_rows=0), truth, 0)
        if k % 2:
            src.free()
        ow = vp(orc.orc_instance_new(sz(N), sz(N), sz(ni), (sz * 3)(*nnz), (ctypes.c_uint64 * len(rows))(*rows), (ctypes.c_uint64 * len(cols))(*cols),
                                     vals, bv, sz(N), bi))
        assert orc.orc_instance_is_sat(ow) == 0, name
        orc.orc_instance_free(ow)
    assert inst.is_sat(inst.vars, inst.inputs) is True       # and the right witness still passes afterwards
    i = list(good_inputs); i[4] = (i[4] + 1) % Q              # an input that no constraint reads: still satisfied, here and for the oracle
    assert _failing_rows(nnz, rows, cols, vals_int, _z(good_vars, i, N), N) == [] and inst.is_sat(inst.vars, mont_bulk(i)) is True
    orc.orc_instance_free(oi); inst.free()


def test_skewed_instance_with_a_long_row(P, ctx, orc):
    num_cons, num_vars, num_inputs = 1 << 12, 1 << 16, 2
    rng = random.Random(2024)
    pool = list(range(64))
    (A, B, C), v, inputs, touching = _skewed_instance(rng, num_cons, num_vars, num_inputs, 300, pool)
    t = num_vars - 1
    assert t not in touching and len(A) > num_vars and len(set((r, c) for r, c, _ in A)) <= len(A) - 2
    ent = A + B + C
    nnz = [len(A), len(B), len(C)]
    rows = (ctypes.c_uint64 * len(ent))(*[e[0] for e in ent]); cols = (ctypes.c_uint64 * len(ent))(*[e[1] for e in ent])
    vals = b"".join(e[2].to_bytes(32, "little") for e in ent)
    inst = P.Instance.new(ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, vals)
    lr, lc, lv = [e[0] for e in ent], [e[1] for e in ent], [e[2] for e in ent]   # num_vars is a power of two above num_inputs + 1: no column shift

    def run(vv, expect):
        truth = _failing_rows(nnz, lr, lc, lv, _z(vv, inputs, num_vars), num_cons)
        assert truth == expect
        bv, bi = mont_bulk(vv), mont_bulk(inputs)
        for src in (bv, P.VarsAssignment(ctx, bv)):
            assert inst.is_sat(src, bi) is (not truth)
            _check_report(inst.check(src, bi, max_rows=num_cons), truth, num_cons)
            _check_report(inst.check(src, bi, max_rows=2), truth, 2)
        err = ctypes.c_int(0)
        oi = vp(orc.orc_instance_new_padded(sz(num_cons), sz(num_vars), sz(num_inputs), (sz * 3)(*nnz), rows, cols, vals, bv, sz(num_vars), bi,
                                            ctypes.byref(err)))
        assert err.value == 0 and oi
        assert orc.orc_instance_is_sat(oi) == (0 if truth else 1)
        orc.orc_instance_free(oi)

    run(v, [])                                                # satisfied as built
    j = max(pool, key=lambda c: len(touching.get(c, ())))     # a variable that several short rows touch
    assert len(touching[j]) >= 3
    w = list(v); w[j] = (w[j] + 1 + rng.randrange(Q - 1)) % Q
    run(w, [0] + sorted(touching[j]))                         # the long row and exactly the short rows that touch it
    w = list(v); w[t] = (w[t] + 1 + rng.randrange(Q - 1)) % Q
    run(w, [0])                                               # the C-side variable alone: only row 0
    w = list(v); w[12345] = (w[12345] + 1) % Q                # a variable that only the long row reads
    assert 12345 not in touching
    run(w, [0])
    inst.free()


def test_padding_and_error_semantics(P, ctx, orc):
    # the instance of test_padded_constraints_like_reference (lib.rs:672-753): 1 constraint, 0 variables, 3 inputs
    num_cons, num_vars, num_inputs = 1, 0, 3
    le = lambda x: (x % Q).to_bytes(32, "little")
    A = [(0, num_vars + 2, le(1))]
    B = [(0, num_vars + 2, le(1))]
    C = [(0, num_vars + 1, le(1)), (0, num_vars, le(-13)), (0, num_vars + 3, le(-1))]
    ent = A + B + C
    nnz = [len(A), len(B), len(C)]
    rows = (ctypes.c_uint64 * len(ent))(*[e[0] for e in ent]); cols = (ctypes.c_uint64 * len(ent))(*[e[1] for e in ent])
    inst = P.Instance.new(ctx, num_cons, num_vars, num_inputs, nnz, rows, cols, b"".join(e[2] for e in ent))
    empty = (ctypes.c_uint64 * 0)()
    assert inst.is_sat(empty, mont_array([16, 1, 2])) is True
    rep = inst.check(empty, mont_array([16, 1, 3]))
    assert inst.is_sat(empty, mont_array([16, 1, 3])) is False
    assert rep.violated == 1 and rep.first_row == 0 and rep.rows == [0]
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        inst.is_sat(empty, mont_array([16, 1]))
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        inst.is_sat(mont_array([1, 2, 3, 4, 5]), mont_array([16, 1, 2]))   # num_vars is padded to 4: five variables are one too many
    inst.free()
    # fewer variables than num_vars are zero-padded (lib.rs:244-252)
    N, ni, seed = 1 << 10, 10, 77
    inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
    nnz, rows, cols, vals, _, _ = _export(orc, oi, N, ni)
    vals_int = from_mont_bulk(vals, sum(nnz))
    v, i = from_mont_bulk(inst.vars, N), from_mont_bulk(inst.inputs, ni)
    short = v[:N - 5]
    truth = _failing_rows(nnz, list(rows), list(cols), vals_int, _z(short, i, N), N)
    assert truth                                              # the five dropped variables are not zero
    for src in (mont_bulk(short), P.VarsAssignment(ctx, mont_bulk(short))):
        assert inst.is_sat(src, inst.inputs) is False
        _check_report(inst.check(src, inst.inputs, max_rows=64), truth, 64)
    # one variable too many, a wrong number of inputs: errors, not False (lib.rs:235-241)
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        inst.is_sat(mont_bulk(v + [1]), inst.inputs)
    with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
        inst.check(P.VarsAssignment(ctx, mont_bulk(v + [1])), inst.inputs)
    for bad in (ni - 1, ni + 1):
        with pytest.raises(P.SpartanHipError, match="InvalidNumberOfInputs"):
            inst.is_sat(inst.vars, mont_bulk((i + [3])[:bad]))
    assert inst.is_sat(inst.vars, inst.inputs) is True       # the context and the instance are still usable
    orc.orc_instance_free(oi); inst.free()


def _oracle_bytes(orc, p):
    n = orc.orc_proof_bytes(p, None, sz(0))
    b = (ctypes.c_uint8 * n)()
    orc.orc_proof_bytes(p, b, sz(n))
    return bytes(b)


def test_check_then_prove_right_and_wrong_witness(P, ctx, orc):
    """The check leaves the context and the proof path as they were: proofs after it equal the oracle's, for the satisfying witness and — what
    nothing fed the device path before — for an unsatisfying one, whose proofs the oracle's verifiers reject."""
    s, seed, ni = 10, 21, 10
    N = 1 << s
    orc.orc_set_threads(ctypes.c_int(1))
    inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
    digest = b"is-sat-digest"
    inst.set_digest(digest)
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
    nnz, rows, cols, vals, _, _ = _export(orc, oi, N, ni)
    gens, ngens = P.SNARKGens(ctx, N, N, ni, N), P.NIZKGens(ctx, N, N, ni)
    enc = P.SNARK.encode(ctx, inst, gens)
    og, ong = vp(orc.orc_snark_gens_new(sz(N), sz(N), sz(ni), sz(N))), vp(orc.orc_nizk_gens_new(sz(N), sz(N), sz(ni)))
    oe = vp(orc.orc_snark_encode(oi, og))
    tape = P.seed_scalar(b"tape", seed)
    wrong = from_mont_bulk(inst.vars, N)
    wrong[N // 2] = (wrong[N // 2] + 1) % Q
    wrong = mont_bulk(wrong)
    ow = vp(orc.orc_instance_new(sz(N), sz(N), sz(ni), (sz * 3)(*nnz), rows, cols, vals, wrong, sz(N), inst.inputs))
    for vars_, o_inst, ok in ((inst.vars, oi, True), (wrong, ow, False)):
        t0 = _trips(ctx)
        assert inst.is_sat(vars_, inst.inputs) is ok
        assert _trips(ctx) == t0 + 1
        rep = inst.check(vars_, inst.inputs)
        assert (rep.violated == 0) is ok and orc.orc_instance_is_sat(o_inst) == (1 if ok else 0)
        got = P.SNARK.prove(ctx, inst, enc, vars_, inst.inputs, gens, b"snark_example", tape)
        op = vp(orc.orc_snark_prove(o_inst, og, oe, b"snark_example", tape, None))
        assert got == _oracle_bytes(orc, op)
        assert orc.orc_snark_verify(op, o_inst, og, oe, b"snark_example") == (1 if ok else 0)
        orc.orc_proof_free(op)
        got = P.NIZK.prove(ctx, inst, vars_, inst.inputs, ngens, b"nizk_example", tape)
        op = vp(orc.orc_nizk_prove(o_inst, ong, digest, sz(len(digest)), b"nizk_example", tape, None))
        assert got == _oracle_bytes(orc, op)
        assert orc.orc_nizk_verify(op, o_inst, ong, digest, sz(len(digest)), b"nizk_example") == (1 if ok else 0)
        orc.orc_proof_free(op)
        va = P.VarsAssignment(ctx, vars_)                     # check, then prove, on the same resident assignment
        assert inst.is_sat(va, inst.inputs) is ok
        assert P.NIZK.prove(ctx, inst, va, inst.inputs, ngens, b"nizk_example", tape) == got
        va.free()
    orc.orc_instance_free(ow); orc.orc_encode_free(oe); orc.orc_snark_gens_free(og); orc.orc_nizk_gens_free(ong); orc.orc_instance_free(oi)
    enc.free(); gens.free(); ngens.free(); inst.free()


def test_row_lengths_around_the_thresholds():
    """sp_r1cs_check through the C ABI on matrices whose rows have 0 .. 2500 entries, a different length in each matrix (a row can be long in one
    matrix and short or empty in the others), a row count that is no multiple of 64, and half of the rows made to hold: the failing rows are
    exactly the other half. Lengths sit on both sides of the kernel's two cuts (one lane up to 32 entries; chunks of 1024)."""
    from spartan_amd import capi
    L = capi.lib
    rng = random.Random(99)
    num_rows, num_cols = 203, 4096
    lens = [0, 1, 2, 31, 32, 33, 63, 64, 65, 200, 1023, 1024, 1025, 2048, 2500]
    zv = [rng.randrange(1, Q) for _ in range(num_cols)]
    mats = [[], [], []]
    expect = []
    for r in range(num_rows):
        sums = []
        for k in range(3):
            n = lens[(r + 4 * k + (r // len(lens)) * (k + 1)) % len(lens)]
            ent = [(r, rng.randrange(num_cols), rng.randrange(Q)) for _ in range(n)]
            mats[k] += ent
            sums.append(sum(x * zv[c] for _, c, x in ent) % Q)
        if r % 2 == 0:     # one more entry of C makes the row hold
            c = rng.randrange(num_cols)
            mats[2].append((r, c, (sums[0] * sums[1] - sums[2]) * pow(zv[c], Q - 2, Q) % Q))
        elif sums[0] * sums[1] % Q != sums[2]:
            expect.append(r)
    assert len(expect) >= num_rows // 2 - 8
    for m in mats:
        rng.shuffle(m)
    ctx = capi.Ctx(0)
    hs = []
    for m in mats:
        h = vp()
        rows = (ctypes.c_uint64 * len(m))(*[e[0] for e in m]); cols = (ctypes.c_uint64 * len(m))(*[e[1] for e in m])
        assert L.sp_sparse_upload(ctx.h, rows, cols, mont_bulk([e[2] for e in m]), sz(len(m)), sz(num_rows), sz(num_cols), ctypes.byref(h)) == 0
        hs.append(h)
    z = capi.Table.upload(ctx, mont_bulk(zv), num_cols)
    nv, first = ctypes.c_uint64(), ctypes.c_uint64()
    out = (ctypes.c_uint64 * num_rows)()
    for _ in range(2):     # the second call runs from the lists the first one built
        assert L.sp_r1cs_check(ctx.h, hs[0], hs[1], hs[2], z.h, ctypes.byref(nv), ctypes.byref(first), out, sz(num_rows)) == 0
        assert nv.value == len(expect) and first.value == expect[0] and list(out[:nv.value]) == expect
    assert L.sp_r1cs_check(ctx.h, hs[0], hs[1], hs[2], z.h, ctypes.byref(nv), ctypes.byref(first), out, sz(5)) == 0
    assert nv.value == len(expect) and list(out[:5]) == expect[:5]
    # every row holds once the odd rows get the same treatment: the count is 0 and the first row is UINT64_MAX
    fix = []
    acc = [[0] * num_rows for _ in range(3)]
    for k in range(3):
        for r, c, x in mats[k]:
            acc[k][r] += x * zv[c]
    for r in expect:
        c = rng.randrange(num_cols)
        fix.append((r, c, (acc[0][r] * acc[1][r] - acc[2][r]) * pow(zv[c], Q - 2, Q) % Q))
    m = mats[2] + fix
    h = vp()
    rows = (ctypes.c_uint64 * len(m))(*[e[0] for e in m]); cols = (ctypes.c_uint64 * len(m))(*[e[1] for e in m])
    assert L.sp_sparse_upload(ctx.h, rows, cols, mont_bulk([e[2] for e in m]), sz(len(m)), sz(num_rows), sz(num_cols), ctypes.byref(h)) == 0
    assert L.sp_r1cs_check(ctx.h, hs[0], hs[1], h, z.h, ctypes.byref(nv), ctypes.byref(first), out, sz(num_rows)) == 0
    assert nv.value == 0 and first.value == 2**64 - 1
    # shapes that do not fit together, a z that is too short: SP_EINVAL
    other = vp()
    assert L.sp_sparse_upload(ctx.h, rows, cols, mont_bulk([e[2] for e in m]), sz(len(m)), sz(num_rows + 1), sz(num_cols), ctypes.byref(other)) == 0
    assert L.sp_r1cs_check(ctx.h, hs[0], hs[1], other, z.h, ctypes.byref(nv), ctypes.byref(first), None, sz(0)) == -1
    zs = capi.Table.upload(ctx, mont_bulk(zv[:num_cols - 1]), num_cols - 1)
    assert L.sp_r1cs_check(ctx.h, hs[0], hs[1], hs[2], zs.h, ctypes.byref(nv), ctypes.byref(first), None, sz(0)) == -1
    for x in hs + [h, other]:
        L.sp_sparse_free(x)
    z.free(); zs.free(); ctx.close()
