"""The SPARK kernel family (spartan_amd/csrc/spark.hip: batched cubic sum-check, product trees, hash layers, dot_many / dot3, gathers and
views) on FIELD EDGE VALUES and at EVERY BOUNDARY OF ITS HOST-SIDE DISPATCH, at small shapes. tests/test_gpu_large.py holds the throughput
shapes on uniform random scalars; here the tables are made of the Fq edge pool of tests/field_vectors.py (layout a: neighbouring lanes
differ; layout c: a whole wavefront of one value), challenges and weights cycle through 0, one, q - 1 and a random residue, one table per
chain has equal halves (x1 - x0 = 0 in every pair), and the case lists below sit on the thresholds of the dispatch:

  tiny / streaming kernels; partial sums added by the host (one block; blocks x instances exactly 320) or by k_reduce_partials_batched (the
  first reachable product above 320); table pointers in the kernel arguments (24 instances) or staged in the host-mapped page (25, 64);
  the 18 sums of the two-rounds kernel added by the host or by k_reduce_partials18, and left in the scratch buffer when 64 instances'
  worth does not fit the result area; short tables handed over (21 instances, ending 192 bytes below TAIL_OFF) or not (22); product trees
  entered at the tail, after a one-layer and after a two-layers launch, in one, two and three chunks of 16 circuits; the eq-factored form
  at its minimum length with and without generic instances and at its cap of 24 instances.

tests/test_spark_reference.py asserts on the CPU (through spark_reference.plan) that the lists reach each of these, so a changed library
constant cannot slide a case off its boundary unnoticed. Expected values: the Python-integer models of tests/spark_reference.py, which
that module checks against the oracle. Every comparison is an exact integer comparison of every output word and every downloaded table
entry, and every value the device returns must be below q. After a SpartanHipError or an unexpected status nothing further is started."""
import ctypes, functools, random
import pytest
from tests import field_vectors as V
from tests import spark_reference as S
from tests.helpers import Q, vp, sz

pytestmark = pytest.mark.gpu

SP_EINVAL = -1
ZERO, ONE, MINUS = 0, S.ONE, Q - 1

# ------------------------------------------------------------------ the case lists (imported by tests/test_spark_reference.py: no GPU needed)
# a. (len0, ninst, shared, layout): instances [0, shared) share one C, the others own theirs
CHAIN_CASES = [
    (2, 1, 0, "a"),            # eval only: bind_eval refuses tables below 4
    (4, 1, 0, "a"),
    (128, 3, 3, "a"),
    (128, 24, 23, "a"),        # the most instances that travel in the kernel arguments
    (256, 64, 63, "a"),        # staged arguments, host-summed
    (1024, 25, 0, "a"),        # staged, host-summed
    (1024, 41, 2, "a"),        # 8 blocks x 41 instances = 328: the first product of a block count and an instance count above 320
    (1024, 64, 32, "a"),       # staged, reduced by kernel
    (1 << 15, 5, 3, "a"),      # streaming -> tiny + reduced -> tiny + host (1280, 640, exactly 320 at quarter 2048) -> one block
    (1 << 15, 5, 3, "c"),
]
# b. (ell, ninst, wstart, layout): wstart None = unweighted, else weight k = cycle[(wstart + k) % 4] of (0, one, q - 1, random)
TWO_ROUND_CASES = (
    [(ell, 1, w, "a") for ell in (1, 2, 3, 4, 5) for w in (None, 0, 2)] +     # one instance: unweighted, weight 0, weight q - 1
    [(ell, 21, 1, "a") for ell in (3, 4, 5)] +                                  # the tables ARE handed over
    [(ell, 22, 1, "a") for ell in (3, 4, 5)] +                                  # ... are not
    [(5, 24, 1, "a"),                                                           # the last inline count
     (6, 25, 1, "a"), (9, 25, 1, "a"),                                          # staged pointers and weights; k_reduce_partials18 at 9
     (4, 64, None, "a"),                                                        # 64 x 18 sums
     (13, 5, 1, "a"), (13, 5, 1, "c")])
# c. (neq, ninst) at EQ_LEN entries
EQ_LEN = 65536
EQ_CASES = [(1, 1), (24, 24), (3, 24)]
# d. (n, count) of sp_product_tree_many_from(.., 0), and n of sp_product_tree
TREE_CASES = [(2, 3), (2048, 16), (2048, 17), (4096, 33), (8192, 2), (16384, 2)]
TREE_SINGLE = [2, 4, 2048, 4096]
# f. the shapes of test_records_and_round_trips_of_every_batched_round_call: the smallest case of the lists above on each side of each branch
RECORD_CHAIN = [(128, 3), (256, 64), (1024, 41), (1 << 15, 5)]      # (len0, ninst) of a.
RECORD_EQ = [(1, 1), (3, 24)]                                       # (neq, ninst) of c.
RECORD_TWO = [(3, 21), (3, 22), (9, 25), (4, 64)]                   # (ell, ninst) of b., weighted as there
# e.
DOT_MANY_CASES = [(nt, n, "edge") for nt in (1, 64) for n in (1, 255, 256, 257, 3000)] + [(64, 257, "minus_one")]

_DEVICE_ERROR = []      # a SpartanHipError or an unexpected status from the library: nothing further is started in this module
COUNTS = {"a": 0, "b": 0, "c": 0, "d": 0, "e": 0}      # exact comparisons (output words and table entries) per section


@pytest.fixture(autouse=True)
def _nothing_after_a_device_error():
    if _DEVICE_ERROR:
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    yield


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    if _DEVICE_ERROR:     # module fixtures are set up before the function-scoped guard above
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    c = capi.Ctx(0)
    yield c
    c.close()
    _packed.cache_clear()
    print("\nexact comparisons per section: %s" % ", ".join("%s %d" % kv for kv in sorted(COUNTS.items())))


def _flags_device_errors(test):
    """a SpartanHipError from the binding stops the module in the same way as an unexpected status"""
    @functools.wraps(test)
    def wrapped(*a, **kw):
        from spartan_amd import capi
        try:
            return test(*a, **kw)
        except capi.SpartanHipError as e:
            _DEVICE_ERROR.append("%s: %s" % (test.__name__, e))
            raise
    return wrapped


def _ok(rc, what):
    if rc != 0:
        _DEVICE_ERROR.append("%s returned %d" % (what, rc))
        pytest.fail(_DEVICE_ERROR[-1])


def _refused(rc, what):
    """the call must return SP_EINVAL; any other status stops the module"""
    if rc != SP_EINVAL:
        if rc != 0:
            _DEVICE_ERROR.append("%s returned %d" % (what, rc))
        pytest.fail("%s returned %d, not SP_EINVAL" % (what, rc))


def _arr(vals):
    return (ctypes.c_uint64 * (4 * len(vals))).from_buffer_copy(V.pack(vals))


def _ints(arr, n=None):
    raw = bytes(arr)
    n = len(raw) // 32 if n is None else n
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


def _same(sec, got, want, what, counts=None):
    """exact comparison of every value, each below q; counts: another module's tally (tests/test_gpu_fq_edges.py)"""
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i] or got[i] >= Q]
    if bad:
        i = bad[0]
        pytest.fail("%s: %d of %d values differ, first at %d\n    want %#066x\n    got  %#066x%s" % (
            what, len(bad), len(want), i, want[i], got[i], "  (not reduced: >= q)" if got[i] >= Q else ""))
    (COUNTS if counts is None else counts)[sec] += len(want)


def _same_table(sec, t, want, what, off=0):
    """the table's length and its full contents (bytes first: the expected values are below q)"""
    n = len(want)
    raw = bytes(t.download(n, off))
    if raw != V.pack(want):
        _same(sec, _ints(raw), want, what)
    COUNTS[sec] += n


@functools.lru_cache(maxsize=None)
def _packed(layout, n, k, nonzero=False):
    vals = (S.nonzero_edge_table if nonzero else S.edge_table)(layout, n, k)
    return vals, _arr(vals)


def _up(ctx, vals, arr=None):
    from spartan_amd import capi
    return capi.Table.upload(ctx, arr if arr is not None else _arr(vals), len(vals))


def _up_edge(ctx, layout, n, k):
    vals, arr = _packed(layout, n, k)
    return vals, _up(ctx, vals, arr)


def _handles(tabs):
    return (vp * len(tabs))(*[t.h for t in tabs])


def _instances(ctx, layout, n, ninst, nd):
    """A_k, B_k and nd distinct C tables from the edge pool; of several instances the LAST one's A has equal halves (x1 - x0 = 0 in every pair
    of the first round). Returns (A, B, C) as lists of residues and (tA, tB, tC) on the device."""
    A, B, C, tA, tB, tC = [], [], [], [], [], []
    for k in range(ninst):
        a, _ = _packed(layout, n, 3 * k)
        if k == ninst - 1 and ninst >= 2 and n >= 4:
            a = a[:n // 2] * 2
            tA.append(_up(ctx, a))
        else:
            tA.append(_up(ctx, a, _packed(layout, n, 3 * k)[1]))
        A.append(a)
        b, t = _up_edge(ctx, layout, n, 3 * k + 1); B.append(b); tB.append(t)
    for j in range(nd):
        c, t = _up_edge(ctx, layout, n, 3 * j + 2); C.append(c); tC.append(t)
    return A, B, C, tA, tB, tC


# ------------------------------------------------------------------ a. one round per trip, a chain across every boundary
@pytest.mark.parametrize("len0,ninst,shared,layout", CHAIN_CASES)
@_flags_device_errors
def test_one_round_chain_crosses_every_dispatch_boundary(ctx, len0, ninst, shared, layout):
    """sp_sumcheck_eval_batched (mutates nothing) against cubic_evals at every length, then sp_sumcheck_bind_eval_batched with the next
    challenge of the cycle: the evaluations, every table's new length and the full contents of every A, B and distinct C; down to length 2,
    where the fused call must refuse (its results are undefined below 4) and leave the tables as they are."""
    from spartan_amd import capi
    L = capi.lib
    nd = (1 if shared else 0) + ninst - shared
    cidx = [0 if k < shared else k - shared + (1 if shared else 0) for k in range(ninst)]
    A, B, C, tA, tB, tC = _instances(ctx, layout, len0, ninst, nd)
    hA, hB, hC = _handles(tA), _handles(tB), _handles([tC[j] for j in cidx])
    chal = S.edge_challenges(len0 + ninst)
    out = (ctypes.c_uint64 * (12 * ninst))()
    evals = lambda: [x for k in range(ninst) for x in S.cubic_evals(A[k], B[k], C[cidx[k]])]
    want, length, j = evals(), len0, 0
    while True:
        what = "len0=%d ninst=%d layout %s at length %d" % (len0, ninst, layout, length)
        _ok(L.sp_sumcheck_eval_batched(ctx.h, hA, hB, hC, sz(ninst), out), "sp_sumcheck_eval_batched " + what)
        _same("a", _ints(out, 3 * ninst), want, "sp_sumcheck_eval_batched " + what)
        if length < 4:
            break
        r = chal[j % 4]; j += 1
        A = [S.bind(a, r) for a in A]; B = [S.bind(b, r) for b in B]; C = [S.bind(c, r) for c in C]
        want = evals()       # of the bound tables: the next eval call must return the same
        _ok(L.sp_sumcheck_bind_eval_batched(ctx.h, hA, hB, hC, sz(ninst), _arr([r]), out), "sp_sumcheck_bind_eval_batched " + what)
        _same("a", _ints(out, 3 * ninst), want, "sp_sumcheck_bind_eval_batched r=%#x %s" % (r, what))
        length //= 2
        for name, tabs, vals in (("A", tA, A), ("B", tB, B), ("C", tC, C)):
            for k, (t, v) in enumerate(zip(tabs, vals)):
                assert len(t) == length, (name, k, what)
                _same_table("a", t, v, "bound %s[%d] r=%#x from %s" % (name, k, r, what))
    _refused(L.sp_sumcheck_bind_eval_batched(ctx.h, hA, hB, hC, sz(ninst), _arr([chal[3]]), out), "sp_sumcheck_bind_eval_batched at length 2")
    for t, v in ((tA[0], A[0]), (tB[-1], B[-1]), (tC[-1], C[-1])):
        assert len(t) == 2
        _same_table("a", t, v, "table after the refused call, len0=%d" % len0)
    for t in tA + tB + tC:
        t.free()


# ------------------------------------------------------------------ b. two rounds per trip
@pytest.mark.parametrize("ell,ninst,wstart,layout", TWO_ROUND_CASES)
@_flags_device_errors
def test_two_round_trips_on_edge_values(ctx, ell, ninst, wstart, layout):
    """sp_sumcheck_eval_coeffs_batched, then trips of sp_sumcheck_bind2_eval_batched (bound tables longer than 16) and
    sp_sumcheck_bind2_eval_tables_batched (16 and below) down to the final claims; all but the last instance share their C. After each trip:
    the evaluations, the coefficients (M0, M3, T1, T2) themselves and through predict() against the mid-round, every bound table, the heads,
    and the handed-over tables - or the all-ones first word where nothing is handed over (more than 8 entries, more than 21 instances)."""
    from spartan_amd import capi
    L = capi.lib
    n = 1 << ell
    nd = 1 if ninst == 1 else 2
    cidx = [0] * (ninst - 1) + [nd - 1]
    A, B, C, tA, tB, tC = _instances(ctx, layout, n, ninst, nd)
    hA, hB, hC = _handles(tA), _handles(tB), _handles([tC[j] for j in cidx])
    cyc = S.edge_challenges(100 * ell + ninst)
    w = None if wstart is None else [cyc[(wstart + k) % 4] for k in range(ninst)]
    assert w is None or 0 in w or ninst == 1      # a single instance is run with weight 0 and, as another case, with weight q - 1
    wm = _arr(w) if w else None
    nout = 1 if w else ninst
    comb = lambda per: S.weighted(per, w) if w else [x for v in per for x in v]
    evals = lambda: comb([S.cubic_evals(A[k], B[k], C[cidx[k]]) for k in range(ninst)])
    coeffs = lambda: comb([S.bind2_coeffs(A[k], B[k], C[cidx[k]]) for k in range(ninst)])
    ev = (ctypes.c_uint64 * (12 * nout))(); co = (ctypes.c_uint64 * (48 * nout))()
    heads = (ctypes.c_uint64 * (4 * (2 * ninst + nd)))(); tables = (ctypes.c_uint64 * (4 * ninst * 3 * 8))()
    tag = "ell=%d ninst=%d w=%s layout %s" % (ell, ninst, wstart, layout)

    def check_trip(length, what, with_tables):
        """the outputs of the trip that left tables of `length`; returns the coefficients it brought"""
        got_co = None
        if length >= 2:
            _same("b", _ints(ev, 3 * nout), evals(), "evaluations, " + what)
        if length >= 4:
            got_co = _ints(co, 12 * nout)
            _same("b", got_co, coeffs(), "coefficients, " + what)
        if length == 1:
            want = [x for k in range(ninst) for x in (A[k][0], B[k][0])] + [c[0] for c in C]
            _same("b", _ints(heads, 2 * ninst + nd), want, "heads, " + what)
        if with_tables:
            if 2 <= length <= 8 and ninst <= 21:      # the header's contract: tables of 2, 4 or 8 entries and at most 21 instances
                want = [x for k in range(ninst) for T in (A[k], B[k], C[cidx[k]]) for x in T]
                _same("b", _ints(tables, 3 * ninst * length), want, "handed-over tables, " + what)
            else:
                assert tables[0] == 0xFFFFFFFFFFFFFFFF, ("first word of out_tables", what)
                COUNTS["b"] += 1
        return got_co

    def check_tables(length, what):
        for name, tabs, vals in (("A", tA, A), ("B", tB, B), ("C", tC, C)):
            for k, (t, v) in enumerate(zip(tabs, vals)):
                assert len(t) == length, (name, k, what)
                _same_table("b", t, v, "bound %s[%d], %s" % (name, k, what))

    length = n
    _ok(L.sp_sumcheck_eval_coeffs_batched(ctx.h, hA, hB, hC, sz(ninst), wm, ev, co if n >= 4 else None), "sp_sumcheck_eval_coeffs_batched " + tag)
    c12 = check_trip(length, "sp_sumcheck_eval_coeffs_batched " + tag, False)
    if n <= 16:     # the same trip through the call that hands the tables over (no bind)
        _ok(L.sp_sumcheck_bind2_eval_tables_batched(ctx.h, hA, hB, hC, sz(ninst), None, None, wm, ev, co if n >= 4 else None, None, tables),
            "sp_sumcheck_bind2_eval_tables_batched without a bind, " + tag)
        c12 = check_trip(length, "sp_sumcheck_bind2_eval_tables_batched without a bind, " + tag, True)
        check_tables(length, "after the trips without a bind, " + tag)
    j = 0
    while length >= 2:
        r0 = cyc[j % 4]
        r1 = cyc[(j + 1) % 4] if length >= 4 else None      # an odd number of variables: the last trip binds once
        j += 1
        what = "bind at (%s, %s) from length %d, %s" % (hex(r0), hex(r1) if r1 is not None else None, length, tag)
        A = [S.bind(a, r0) for a in A]; B = [S.bind(b, r0) for b in B]; C = [S.bind(c, r0) for c in C]
        length //= 2
        if r1 is not None:
            _same("b", S.predict(c12, r0), evals(), "mid-round predicted from the coefficients, " + what)     # the cubic predicts the round after the bind at r0
            A = [S.bind(a, r1) for a in A]; B = [S.bind(b, r1) for b in B]; C = [S.bind(c, r1) for c in C]
            length //= 2
        pe, pc, ph = ev if length >= 2 else None, co if length >= 4 else None, heads if length == 1 else None
        with_tables = length <= 16
        if with_tables:
            _ok(L.sp_sumcheck_bind2_eval_tables_batched(ctx.h, hA, hB, hC, sz(ninst), _arr([r0]), _arr([r1]) if r1 is not None else None, wm, pe, pc, ph, tables),
                "sp_sumcheck_bind2_eval_tables_batched " + what)
        else:
            _ok(L.sp_sumcheck_bind2_eval_batched(ctx.h, hA, hB, hC, sz(ninst), _arr([r0]), _arr([r1]) if r1 is not None else None, wm, pe, pc, ph),
                "sp_sumcheck_bind2_eval_batched " + what)
        c12 = check_trip(length, what, with_tables)
        check_tables(length, what)
    assert length == 1
    for t in tA + tB + tC:
        t.free()


# ------------------------------------------------------------------ c. the eq table as a factor, at its limits
def _eq_tables(ctx, neq, ninst):
    n = EQ_LEN
    A, B, tA, tB = [], [], [], []
    for k in range(ninst):
        a, t = _up_edge(ctx, "a" if k % 2 == 0 else "c", n, 2 * k); A.append(a); tA.append(t)
        b, t = _up_edge(ctx, "a", n, 2 * k + 1); B.append(b); tB.append(t)
    Ceq, tCeq = _up_edge(ctx, "a", n, 2 * ninst)
    Cg, tCg = [], []
    for k in range(ninst - neq):
        c, t = _up_edge(ctx, "c" if k % 2 == 0 else "a", n, 2 * ninst + 1 + k); Cg.append(c); tCg.append(t)
    return A, B, Ceq, Cg, tA, tB, tCeq, tCg


def _eq_want(A, B, Ceq, Cg, neq):
    w = []
    for k in range(len(A)):
        w += S.quad_eq(A[k], B[k], Ceq) + [0, 0] if k < neq else S.cubic_evals4(A[k], B[k], Cg[k - neq])
    return w


@pytest.mark.parametrize("which", ["eval", "r=0", "r=q-1", "r=random"])
@pytest.mark.parametrize("neq,ninst", EQ_CASES)
@_flags_device_errors
def test_eq_factored_form_at_its_limits(ctx, neq, ninst, which):
    """sp_sumcheck_eval_batched_eq / sp_sumcheck_bind_eval_batched_eq at 65536 entries, the shortest tables the form takes, with no generic
    launch (neq = ninst), one, and the cap of 24 instances. "eval": the evaluation and the refusal of 25 instances, no table touched. The others:
    a bind at that r on freshly uploaded tables, after which the eq table must come back unchanged, with its length; after r = 0 also the
    refusal of a second bind (32768 < 65536), then sp_table_scale_prefix at k = q - 1, one, 0 with n < len.
    Measured on an MI355X host: (3, 24) takes 0.9 s ("eval") to 1.1 s (a bind), nearly all of it the Python reference of the 21 generic
    instances; the slowest case of test_gpu_field_lanes.py::test_sumcheck_kernels_on_edge_tables took 0.09 s in the same session. 24 is kept:
    it is the cap the case is there for."""
    from spartan_amd import capi
    L = capi.lib
    n = EQ_LEN
    A, B, Ceq, Cg, tA, tB, tCeq, tCg = _eq_tables(ctx, neq, ninst)
    hA, hB, hC = _handles(tA), _handles(tB), _handles([tCeq] * neq + tCg)
    out = (ctypes.c_uint64 * (16 * ninst))()
    tag = "neq=%d ninst=%d" % (neq, ninst)
    if which == "eval":
        _ok(L.sp_sumcheck_eval_batched_eq(ctx.h, hA, hB, hC, sz(ninst), sz(neq), out), "sp_sumcheck_eval_batched_eq " + tag)
        _same("c", _ints(out, 4 * ninst), _eq_want(A, B, Ceq, Cg, neq), "sp_sumcheck_eval_batched_eq " + tag)
        if ninst == S.EQ_MAX_INST:      # one instance more than the kernel arguments hold: refused before any table is touched
            h25 = lambda tabs: _handles(tabs + [tabs[-1]])
            o25 = (ctypes.c_uint64 * (16 * 25))()
            c25 = [tCeq] * neq + tCg + [tCg[-1] if tCg else tCeq]
            n25 = neq if tCg else neq + 1
            _refused(L.sp_sumcheck_eval_batched_eq(ctx.h, h25(tA), h25(tB), _handles(c25), sz(25), sz(n25), o25), "sp_sumcheck_eval_batched_eq with 25 instances")
            _refused(L.sp_sumcheck_bind_eval_batched_eq(ctx.h, h25(tA), h25(tB), _handles(c25), sz(25), sz(n25), _arr([ONE]), o25),
                     "sp_sumcheck_bind_eval_batched_eq with 25 instances")
        assert all(len(t) == n for t in tA + tB + tCg + [tCeq])
        for t, v in ((tA[-1], A[-1]), (tB[0], B[0]), (tCeq, Ceq)) + (((tCg[-1], Cg[-1]),) if tCg else ()):
            _same_table("c", t, v, "table after the evaluation and the refused calls, " + tag)
        for t in tA + tB + tCg + [tCeq]:
            t.free()
        return
    r = {"r=0": ZERO, "r=q-1": MINUS, "r=random": random.Random(neq * 100 + ninst).randrange(Q)}[which]
    A = [S.bind(a, r) for a in A]; B = [S.bind(b, r) for b in B]; Cg = [S.bind(c, r) for c in Cg]
    _ok(L.sp_sumcheck_bind_eval_batched_eq(ctx.h, hA, hB, hC, sz(ninst), sz(neq), _arr([r]), out), "sp_sumcheck_bind_eval_batched_eq r=%#x %s" % (r, tag))
    _same("c", _ints(out, 4 * ninst), _eq_want(A, B, Ceq, Cg, neq), "sp_sumcheck_bind_eval_batched_eq r=%#x %s" % (r, tag))
    for name, tabs, vals in (("A", tA, A), ("B", tB, B), ("C", tCg, Cg)):
        for k, (t, v) in enumerate(zip(tabs, vals)):
            assert len(t) == n // 2, (name, k, tag)
            _same_table("c", t, v, "bound %s[%d] r=%#x %s" % (name, k, r, tag))
    assert len(tCeq) == n
    _same_table("c", tCeq, Ceq, "the eq table after the bind (read, never written), " + tag)
    if which == "r=0":
        _refused(L.sp_sumcheck_bind_eval_batched_eq(ctx.h, hA, hB, hC, sz(ninst), sz(neq), _arr([r]), out), "a second factored bind (32768 entries)")
        assert len(tA[0]) == n // 2 and len(tCeq) == n
        _same_table("c", tA[0], A[0], "A[0] after the refused bind, " + tag)
        m = n
        for k in (MINUS, ONE, ZERO):      # the hand-over: t[i] *= k for i < m, m becomes the length
            m //= 2
            _ok(L.sp_table_scale_prefix(ctx.h, tCeq.h, sz(m), _arr([k])), "sp_table_scale_prefix k=%#x" % k)
            Ceq = [S.mm(x, k) for x in Ceq[:m]]
            assert len(tCeq) == m
            _same_table("c", tCeq, Ceq, "sp_table_scale_prefix k=%#x n=%d" % (k, m))
    for t in tA + tB + tCg + [tCeq]:
        t.free()


# ------------------------------------------------------------------ f. what a batched round call leaves behind
# (call, shape...) -> (round trips by sp_ctx_trips, {profile family: (records, alg_bytes)} of every family the call left a record in).
# MEASURED, not derived from the code under test: this test printed the table on the library as it stood before the batched rounds were
# given one plan and one launch path, and it was written down here as literals. The calls must go on leaving exactly this behind.
CALL_RECORDS = {
    ('eval', 128, 3): (1, {'sumcheck_eval': (1, 36864.0)}),
    ('bind_eval', 128, 3): (1, {'sumcheck_bind_eval': (1, 49152.0)}),
    ('eval', 256, 64): (1, {'sumcheck_eval': (1, 1572864.0)}),
    ('bind_eval', 256, 64): (1, {'sumcheck_bind_eval': (1, 2097152.0)}),
    ('eval', 1024, 41): (1, {'sumcheck_eval': (1, 4030464.0), 'fq_reduce': (1, 31488.0)}),
    ('bind_eval', 1024, 41): (1, {'sumcheck_bind_eval': (1, 5373952.0), 'fq_reduce': (1, 31488.0)}),
    ('eval', 32768, 5): (1, {'sumcheck_eval': (1, 15728640.0), 'fq_reduce': (1, 30720.0)}),
    ('bind_eval', 32768, 5): (1, {'sumcheck_bind_eval': (1, 20971520.0), 'fq_reduce': (1, 122880.0)}),
    ('eq_eval', 65536, 1, 1): (1, {'sumcheck_eval': (1, 5242880.0), 'fq_reduce': (1, 16384.0)}),
    ('eq_bind_eval', 65536, 1, 1): (1, {'sumcheck_bind_eval': (1, 6815744.0), 'fq_reduce': (1, 8192.0)}),
    ('eq_eval', 65536, 3, 24): (1, {'sumcheck_eval': (1, 147849216.0), 'fq_reduce': (1, 393216.0)}),
    ('eq_bind_eval', 65536, 3, 24): (1, {'sumcheck_bind_eval': (1, 196608000.0), 'fq_reduce': (1, 196608.0)}),
    ('eval_coeffs', 3, 21): (1, {'sumcheck_eval': (1, 16128.0)}),
    ('tables, no bind', 3, 21): (1, {'sumcheck_eval': (1, 16128.0)}),
    ('bind2_eval', 3, 21): (1, {'sumcheck_bind_eval': (1, 16128.0)}),
    ('tables', 3, 21): (1, {'sumcheck_bind_eval': (1, 16128.0)}),
    ('eval_coeffs', 3, 22): (1, {'sumcheck_eval': (1, 16896.0)}),
    ('tables, no bind', 3, 22): (1, {'sumcheck_eval': (1, 16896.0)}),
    ('bind2_eval', 3, 22): (1, {'sumcheck_bind_eval': (1, 16896.0)}),
    ('tables', 3, 22): (1, {'sumcheck_bind_eval': (1, 16896.0)}),
    ('eval_coeffs', 9, 25): (1, {'sumcheck_eval': (1, 1228800.0), 'fq_reduce': (1, 230400.0)}),
    ('tables, no bind', 9, 25): (1, {'sumcheck_eval': (1, 1228800.0), 'fq_reduce': (1, 230400.0)}),
    ('bind2_eval', 9, 25): (1, {'sumcheck_bind_eval': (1, 1228800.0), 'fq_reduce': (1, 57600.0)}),
    ('tables', 9, 25): (1, {'sumcheck_bind_eval': (1, 1228800.0), 'fq_reduce': (1, 57600.0)}),
    ('eval_coeffs', 4, 64): (1, {'sumcheck_eval': (1, 98304.0), 'fq_reduce': (1, 36864.0)}),
    ('tables, no bind', 4, 64): (1, {'sumcheck_eval': (1, 98304.0), 'fq_reduce': (1, 36864.0)}),
    ('bind2_eval', 4, 64): (1, {'sumcheck_bind_eval': (1, 98304.0), 'fq_reduce': (1, 36864.0)}),
    ('tables', 4, 64): (1, {'sumcheck_bind_eval': (1, 98304.0), 'fq_reduce': (1, 36864.0)}),
}


@_flags_device_errors
def test_records_and_round_trips_of_every_batched_round_call(ctx):
    """Every entry point of the batched cubic family at the shapes of RECORD_CHAIN / RECORD_EQ / RECORD_TWO, each on freshly uploaded
    tables: the round trips the call makes and the profile records it leaves (how many per family, and their algorithmic bytes) are
    those of CALL_RECORDS - one trip per call, one sumcheck record per round, one fq_reduce record exactly where the sums are added on
    the device. The values the calls return are the other tests' business: every table here holds the same edge values."""
    from spartan_amd import capi
    L = capi.lib
    got = {}

    def fresh(n, ninst, nd):
        """A_k, B_k and nd distinct C (all but the last instance share the first; nd = 1: all share it), as handle arrays"""
        arr = _packed("a", n, 0)[1]
        tabs = [capi.Table.upload(ctx, arr, n) for _ in range(2 * ninst + nd)]
        tC = tabs[2 * ninst:]
        return tabs, _handles(tabs[:ninst]), _handles(tabs[ninst:2 * ninst]), _handles([tC[0]] * (ninst - 1) + [tC[-1]])

    def record(key, call, tabs):
        ctx.prof_reset()
        t0 = L.sp_ctx_trips(ctx.h)
        _ok(call(), repr(key))
        trips = L.sp_ctx_trips(ctx.h) - t0
        got[key] = (trips, {n: (v["launches"], v["alg_bytes"]) for n, v in ctx.prof_read().items() if v["launches"] or v["alg_bytes"]})
        for t in tabs:
            t.free()

    r0, r1 = _arr([S.edge_challenges(1)[3]]), _arr([S.edge_challenges(2)[3]])
    ctx.prof_enable(True)
    try:
        for n, ninst in RECORD_CHAIN:
            out = (ctypes.c_uint64 * (12 * ninst))()
            tabs, hA, hB, hC = fresh(n, ninst, 2)
            record(("eval", n, ninst), lambda: L.sp_sumcheck_eval_batched(ctx.h, hA, hB, hC, sz(ninst), out), tabs)
            tabs, hA, hB, hC = fresh(n, ninst, 2)
            record(("bind_eval", n, ninst), lambda: L.sp_sumcheck_bind_eval_batched(ctx.h, hA, hB, hC, sz(ninst), r0, out), tabs)
        for neq, ninst in RECORD_EQ:
            out = (ctypes.c_uint64 * (16 * ninst))()
            for call in ("eq_eval", "eq_bind_eval"):
                arr = _packed("a", EQ_LEN, 0)[1]
                tabs = [capi.Table.upload(ctx, arr, EQ_LEN) for _ in range(2 * ninst + 1 + ninst - neq)]
                hA, hB, hC = _handles(tabs[:ninst]), _handles(tabs[ninst:2 * ninst]), _handles([tabs[2 * ninst]] * neq + tabs[2 * ninst + 1:])
                if call == "eq_eval":
                    record((call, EQ_LEN, neq, ninst), lambda: L.sp_sumcheck_eval_batched_eq(ctx.h, hA, hB, hC, sz(ninst), sz(neq), out), tabs)
                else:
                    record((call, EQ_LEN, neq, ninst), lambda: L.sp_sumcheck_bind_eval_batched_eq(ctx.h, hA, hB, hC, sz(ninst), sz(neq), r0, out), tabs)
        for ell, ninst in RECORD_TWO:
            n = 1 << ell
            wstart = [w for e, i, w, _ in TWO_ROUND_CASES if (e, i) == (ell, ninst)][0]
            wm = None if wstart is None else _arr([S.edge_challenges(ell)[(wstart + k) % 4] for k in range(ninst)])
            nout = 1 if wm else ninst
            ev = (ctypes.c_uint64 * (12 * nout))(); co = (ctypes.c_uint64 * (48 * nout))()
            heads = (ctypes.c_uint64 * (4 * (2 * ninst + 2)))(); tables = (ctypes.c_uint64 * (4 * ninst * 3 * 8))()
            pc = co if (n >> 2) >= 4 else None      # the coefficients exist for bound tables of 4 entries and more
            tabs, hA, hB, hC = fresh(n, ninst, 2)
            record(("eval_coeffs", ell, ninst), lambda: L.sp_sumcheck_eval_coeffs_batched(ctx.h, hA, hB, hC, sz(ninst), wm, ev, co), tabs)
            tabs, hA, hB, hC = fresh(n, ninst, 2)
            record(("tables, no bind", ell, ninst), lambda: L.sp_sumcheck_bind2_eval_tables_batched(ctx.h, hA, hB, hC, sz(ninst), None, None, wm, ev, co, None, tables), tabs)
            tabs, hA, hB, hC = fresh(n, ninst, 2)
            record(("bind2_eval", ell, ninst), lambda: L.sp_sumcheck_bind2_eval_batched(ctx.h, hA, hB, hC, sz(ninst), r0, r1, wm, ev, pc, heads), tabs)
            tabs, hA, hB, hC = fresh(n, ninst, 2)
            record(("tables", ell, ninst), lambda: L.sp_sumcheck_bind2_eval_tables_batched(ctx.h, hA, hB, hC, sz(ninst), r0, r1, wm, ev, pc, heads, tables), tabs)
    finally:
        ctx.prof_enable(False)
    for key in got:
        print("    %r: %r," % (key, got[key]))
    assert got == CALL_RECORDS


# ------------------------------------------------------------------ d. product trees and hash layers
def _store(ctx, leaves, arr=None):
    """a circuit's store: 2 n entries, the leaves in front, zeros behind"""
    from spartan_amd import capi
    t = capi.Table.alloc(ctx, 2 * len(leaves))
    _ok(capi.lib.sp_table_write(ctx.h, t.h, sz(0), arr if arr is not None else _arr(leaves), sz(len(leaves))), "sp_table_write")
    return t


@pytest.mark.parametrize("n", TREE_SINGLE)
@_flags_device_errors
def test_product_tree_of_one_circuit(ctx, n):
    from spartan_amd import capi
    leaves, arr = _packed("a", n, 7, True)
    t = _store(ctx, leaves, arr)
    _ok(capi.lib.sp_product_tree(ctx.h, t.h, sz(n)), "sp_product_tree n=%d" % n)
    _same_table("d", t, S.product_layers(leaves) + [0, 0], "sp_product_tree n=%d: the store, layer behind layer, and the two unused entries" % n)
    t.free()


@pytest.mark.parametrize("n,count", TREE_CASES)
@_flags_device_errors
def test_product_trees_of_many_circuits(ctx, n, count):
    """sp_product_tree_many_from(.., 0): no launch at all (n = 2), the one-workgroup tail entered directly (2048), after a one-layer launch
    (4096), after a two-layers launch (8192) and after both (16384); 16 circuits per chunk: 16, 17 (a second chunk of one) and 33 (three)"""
    from spartan_amd import capi
    stores, leaves = [], []
    for k in range(count):
        lv, arr = _packed("a" if k % 2 == 0 else "c", n, k, True)
        leaves.append(lv); stores.append(_store(ctx, lv, arr))
    _ok(capi.lib.sp_product_tree_many_from(ctx.h, _handles(stores), sz(count), sz(n), sz(0)), "sp_product_tree_many_from n=%d count=%d" % (n, count))
    for k in range(count):
        _same_table("d", stores[k], S.product_layers(leaves[k]) + [0, 0], "circuit %d of %d, n=%d" % (k, count, n))
    for t in stores:
        t.free()


@_flags_device_errors
def test_product_tree_with_exactly_one_zero_leaf(ctx):
    """only the entries on the zero leaf's path to its root are zero; every other entry is the product of non-zero leaves"""
    from spartan_amd import capi
    n, z = 4096, 2048 + 1365
    leaves = list(_packed("a", n, 11, True)[0])
    leaves[z] = 0
    t = _store(ctx, leaves)
    _ok(capi.lib.sp_product_tree_many_from(ctx.h, _handles([t]), sz(1), sz(n), sz(0)), "sp_product_tree_many_from, one zero leaf")
    want = S.product_layers(leaves)
    path, off, ln, i = set(), 0, n, z
    while True:
        path.add(off + i)
        if ln == 2:
            break
        off += ln; ln //= 2; i %= ln
    assert {i for i, x in enumerate(want) if x == 0} == path and len(path) == 12      # the model itself: one entry per layer
    _same_table("d", t, want + [0, 0], "store with one zero leaf")
    t.free()


HASH_R = [(0, 3), (1, 2), (2, 1), (3, 0)]      # (r_hash, r_multiset) as indices into the cycle (0, one, q - 1, random)


@pytest.mark.parametrize("n", [4, 4096])
@_flags_device_errors
def test_hash_layers_on_edge_values(ctx, n):
    """sp_hash_layer (identity / table addresses, without / with timestamps, ts_inc = 1) and sp_hash_layer_first in both forms (one circuit;
    the read and the write set of one matrix from one pass), then the rest of both trees from layer 1 on"""
    from spartan_amd import capi
    L = capi.lib
    addr, taddr = _up_edge(ctx, "a", n, 31)
    val, tval = _up_edge(ctx, "c" if n > 64 else "a", n, 32)
    ts, tts = _up_edge(ctx, "a", n, 33)
    cyc = S.edge_challenges(n)
    dst = capi.Table.alloc(ctx, n + 7)
    da, db = capi.Table.alloc(ctx, 2 * n), capi.Table.alloc(ctx, 2 * n)
    ident = [S.index_residue(i) for i in range(n)]
    for ih, im in HASH_R:
        rh, rm = cyc[ih], cyc[im]
        for use_addr, use_ts, inc in ((False, False, 0), (True, True, 1), (False, True, 1), (True, False, 0)):
            what = "n=%d r_hash=%#x r_multiset=%#x addr=%s ts=%s inc=%d" % (n, rh, rm, use_addr, use_ts, inc)
            _ok(L.sp_hash_layer(ctx.h, taddr.h if use_addr else None, tval.h, tts.h if use_ts else None, ctypes.c_int(inc), sz(n), _arr([rh]), _arr([rm]),
                                dst.h, sz(7)), "sp_hash_layer " + what)
            want = [S.hash_leaf(addr[i] if use_addr else ident[i], val[i], ts[i] if use_ts else 0, inc, rh, rm) for i in range(n)]
            _same_table("d", dst, want, "sp_hash_layer " + what, off=7)
        _same_table("d", dst, [0] * 7, "the entries in front of dst_off")
        h = n // 2
        for pair, inc in ((False, 0), (False, 1), (True, 0)):
            what = "n=%d r_hash=%#x r_multiset=%#x pair=%s inc=%d" % (n, rh, rm, pair, inc)
            _ok(L.sp_hash_layer_first(ctx.h, taddr.h, tval.h, tts.h, ctypes.c_int(inc), sz(n), _arr([rh]), _arr([rm]), da.h, db.h if pair else None),
                "sp_hash_layer_first " + what)
            lv = [S.hash_leaf(addr[i], val[i], ts[i], inc, rh, rm) for i in range(n)]
            _same_table("d", da, lv + [S.mm(lv[i], lv[h + i]) for i in range(h)], "sp_hash_layer_first, leaves and layer 1, " + what)
            if pair:
                lw = [S.hash_leaf(addr[i], val[i], ts[i], 1, rh, rm) for i in range(n)]
                _same_table("d", db, lw + [S.mm(lw[i], lw[h + i]) for i in range(h)], "sp_hash_layer_first, the write set, " + what)
                _ok(L.sp_product_tree_many_from(ctx.h, _handles([da, db]), sz(2), sz(n), sz(1)), "sp_product_tree_many_from(.., 1) " + what)
                _same_table("d", da, S.product_layers(lv), "the read set's tree, " + what)
                _same_table("d", db, S.product_layers(lw), "the write set's tree, " + what)
    for t in (taddr, tval, tts, dst, da, db):
        t.free()


# ------------------------------------------------------------------ e. reductions, gathers and views
@pytest.mark.parametrize("nt,n,chi_kind", DOT_MANY_CASES)
@_flags_device_errors
def test_dot_many_sizes_and_table_counts(ctx, nt, n, chi_kind):
    from spartan_amd import capi
    chi = [MINUS] * n if chi_kind == "minus_one" else _packed("a", n, 90)[0]
    tchi = _up(ctx, chi)
    T, tT = zip(*[_up_edge(ctx, "a" if k % 2 == 0 else "c", n, k) for k in range(nt)])
    out = (ctypes.c_uint64 * (4 * nt))()
    _ok(capi.lib.sp_dot_many(ctx.h, tchi.h, _handles(list(tT)), sz(nt), out), "sp_dot_many nt=%d n=%d" % (nt, n))
    _same("e", _ints(out, nt), S.dot_many(chi, T), "sp_dot_many nt=%d n=%d chi %s" % (nt, n, chi_kind))
    for t in list(tT) + [tchi]:
        t.free()


@_flags_device_errors
def test_dot3_and_dot3_many(ctx):
    from spartan_amd import capi
    L = capi.lib
    off = 5
    o4 = (ctypes.c_uint64 * 4)()
    for n in (1, 1025):
        T, tT = zip(*[_up_edge(ctx, "a", off + n, 40 + k) for k in range(3)])
        _ok(L.sp_dot3(ctx.h, tT[0].h, tT[1].h, tT[2].h, sz(off), sz(n), o4), "sp_dot3 off=%d n=%d" % (off, n))
        _same("e", _ints(o4, 1), [S.dot3(T[0][off:], T[1][off:], T[2][off:])], "sp_dot3 off=%d n=%d" % (off, n))
        _refused(L.sp_dot3(ctx.h, tT[0].h, tT[1].h, tT[2].h, sz(off + 1), sz(n), o4), "sp_dot3 past the end of its tables")
        for t in tT:
            t.free()
    nt, n = 64, 257
    T, tT = zip(*[_up_edge(ctx, "a" if k % 3 else "c", n, k) for k in range(3 * nt)])
    out = (ctypes.c_uint64 * (4 * nt))()
    _ok(L.sp_dot3_many(ctx.h, _handles(list(tT[:nt])), _handles(list(tT[nt:2 * nt])), _handles(list(tT[2 * nt:])), sz(nt), sz(n), out), "sp_dot3_many")
    _same("e", _ints(out, nt), [S.dot3(T[k], T[nt + k], T[2 * nt + k]) for k in range(nt)], "sp_dot3_many nt=64 n=257")
    for t in tT:
        t.free()


@_flags_device_errors
def test_indices_and_gathers(ctx):
    from spartan_amd import capi
    L = capi.lib
    ix = vp()
    _refused(L.sp_index_upload(ctx.h, (ctypes.c_uint64 * 2)(1, 1 << 32), sz(2), ctypes.byref(ix)), "sp_index_upload of 2^32")
    big = [0, 1, (1 << 32) - 1]
    _ok(L.sp_index_upload(ctx.h, (ctypes.c_uint64 * 3)(*big), sz(3), ctypes.byref(ix)), "sp_index_upload of 2^32 - 1")
    f = capi.Table.alloc(ctx, 5)
    _ok(L.sp_table_from_index(ctx.h, ix, f.h, sz(1)), "sp_table_from_index")
    _same_table("e", f, [0] + [S.index_residue(i) for i in big] + [0], "sp_table_from_index on 0, 1, 2^32 - 1")
    L.sp_index_free(ix)
    f.free()
    n = 300
    mem, tmem = _up_edge(ctx, "a", n, 50)
    for name, addrs in (("every address the same cell", [77] * n), ("addresses descending", list(range(n - 1, -1, -1)))):
        ix = vp()
        _ok(L.sp_index_upload(ctx.h, (ctypes.c_uint64 * n)(*addrs), sz(n), ctypes.byref(ix)), "sp_index_upload")
        g = capi.Table.alloc(ctx, n + 3)
        _ok(L.sp_gather(ctx.h, tmem.h, ix, g.h, sz(3)), "sp_gather, " + name)
        _same_table("e", g, [0, 0, 0] + [mem[a] for a in addrs], "sp_gather, " + name)
        L.sp_index_free(ix)
        g.free()
    tmem.free()


@_flags_device_errors
def test_table_views(ctx):
    """sp_table_view: a window on a parent's storage, not owned"""
    from spartan_amd import capi
    L = capi.lib
    n, off, ln = 1000, 123, 500
    P, tP = _up_edge(ctx, "a", n, 60)
    h = vp()
    _refused(L.sp_table_view(ctx.h, tP.h, sz(600), sz(500), ctypes.byref(h)), "sp_table_view past the parent's capacity")
    _ok(L.sp_table_view(ctx.h, tP.h, sz(off), sz(ln), ctypes.byref(h)), "sp_table_view")
    view = capi.Table(ctx, h)
    assert len(view) == ln
    _same_table("e", view, P[off:off + ln], "the view downloads the parent's slice")
    chi, tchi = _up_edge(ctx, "c", ln, 61)
    out = (ctypes.c_uint64 * 8)()
    _ok(L.sp_dot_many(ctx.h, tchi.h, _handles([view, tP]), sz(2), out), "sp_dot_many on a view")
    _same("e", _ints(out, 2), S.dot_many(chi, [P[off:off + ln], P[:ln]]), "sp_dot_many on a view and on its parent")
    view.free()
    assert len(tP) == n
    _same_table("e", tP, P, "the parent after its view was freed")
    tP.free(); tchi.free()
