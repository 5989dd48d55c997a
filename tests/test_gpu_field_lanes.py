"""The DEVICE forms of the field and curve arithmetic (spartan_amd/csrc/field.hpp: the interleaved carry chains of fq/fp add and sub, the
v_mad_u64_u32 column accumulators of fq_mul / fp_mul / fp_sqr) lane by lane against Python integers, on the vectors of tests/field_vectors.py
that take the rare carry paths, in lane layouts where neighbouring lanes of a wavefront carry differently:

  (a) every class shuffled together with uniform fillers     (b) one edge vector at lane 0, 1, 31, 32, 33, 62, 63 among 63 random lanes
  (c) a whole wavefront of one edge vector                    (d) sizes 1, 63, 64, 65, 255, 257, every class at every size
  (e) divergent: lanes picked by a 64-bit pattern run the operation, the others a different one, under complementary EXEC masks

Every comparison is an exact integer comparison of every lane. The microkernels (tests/csrc/devcheck.hip) exist in a second build with the
generic u128 forms on the same device; it runs the same vectors (layout (a)), and on a mismatch of the device forms it is asked about the
failing elements so the message says whether the kernel or the harness is at fault. Then the product's own kernels (the same inline
assembly in its real surroundings) on tables made of the edge values, against Python formulas and the oracle.

Vectors per operation, all layouts and the divergent runs together: Fq 38 888 (44 classes), Fp 33 679 (31 classes), points 6 879 (7 classes);
the generic build runs layout (a) once more (1 484 / 2 224 / 248)."""
import ctypes, random
import pytest
from tests import field_vectors as V
from tests.helpers import *

pytestmark = pytest.mark.gpu

_DEVICE_ERROR = []      # a non-zero hipError_t from any dc_* call: nothing further is started in this module


@pytest.fixture(autouse=True)
def _nothing_after_a_device_error():
    if _DEVICE_ERROR:
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    yield


@pytest.fixture(scope="module")
def dc():
    return load_devcheck(False)


@pytest.fixture(scope="module")
def dcg():
    return load_devcheck(True)


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    if _DEVICE_ERROR:     # module fixtures are set up before the function-scoped guard above: no context is opened after a device error
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    c = capi.Ctx(0)
    yield c
    c.close()


def _flags_device_errors(test):
    """an error code from the product library stops the module in the same way as one from the microkernels"""
    import functools

    @functools.wraps(test)
    def wrapped(*a, **kw):
        from spartan_amd import capi
        try:
            return test(*a, **kw)
        except capi.SpartanHipError as e:
            _DEVICE_ERROR.append("%s: %s" % (test.__name__, e))
            raise
    return wrapped


def _run(L, op, vec, mode=0, pattern=0):
    n = len(vec)
    rc, out = dc_call(L, op, V.pack([a for _, a, _ in vec]), V.pack([b for _, _, b in vec]), n, mode, pattern)
    if rc != 0:
        _DEVICE_ERROR.append("dc_%s(n=%d, mode=%d, pattern=%#x) returned hipError_t %d" % (op, n, mode, pattern, rc))
        pytest.fail(_DEVICE_ERROR[0])
    return [int.from_bytes(out[32 * i:32 * i + 32], "little") for i in range(n)]


def _check(L, Lother, op, vec, what, mode=0, pattern=0):
    """device output == Python expectation on every lane; the failure message lists each differing lane (first 12 in full)"""
    got = _run(L, op, vec, mode, pattern)
    want = V.expected(op, vec, mode, pattern)
    bad = [i for i in range(len(vec)) if got[i] != want[i]]
    if op.startswith("fq_"):
        bad = sorted(set(bad) | {i for i in range(len(vec)) if got[i] >= Q})    # Fq limbs are always fully reduced
    if not bad:
        return len(vec)
    other = _run(Lother, op, vec, mode, pattern) if Lother is not None else None
    lines = []
    for i in bad[:12]:
        name, a, b = vec[i]
        ran = op if (mode == 0 or (pattern >> (i & 63)) & 1) else V.OPS[op][1]
        lines.append("%s (lane ran %s) class %s element %d = wavefront %d lane %d\n    a = %#066x\n    b = %#066x\n    want %#066x\n    got  %#066x%s\n    %s" % (
            op, ran, name, i, i // 64, i & 63, a, b, want[i], got[i], "  (not reduced: >= q)" if op.startswith("fq_") and got[i] >= Q else "",
            "no second build asked" if other is None else "the other build (%s forms) %s with Python here" % (
                "generic" if Lother.dc_flags() == 7 else "device", "AGREES" if other[i] == want[i] else "DISAGREES")))
    pytest.fail("%s %s: %d of %d lanes differ (lanes within their wavefronts: %s)\n%s" % (
        op, what, len(bad), len(vec), sorted({i & 63 for i in bad})[:64], "\n".join(lines)))


OPS = sorted(V.OPS)


@pytest.mark.parametrize("op", OPS)
def test_shuffled_classes_a(dc, dcg, op):
    _check(dc, dcg, op, V.layout_a(V.OPS[op][0]), "layout (a)")


@pytest.mark.parametrize("op", OPS)
def test_one_edge_lane_per_wavefront_b(dc, dcg, op):
    _check(dc, dcg, op, V.layout_b(V.OPS[op][0]), "layout (b)")


@pytest.mark.parametrize("op", OPS)
def test_whole_wavefront_of_one_edge_vector_c(dc, dcg, op):
    _check(dc, dcg, op, V.layout_c(V.OPS[op][0]), "layout (c)")


@pytest.mark.parametrize("op", OPS)
def test_partial_wavefronts_and_blocks_d(dc, dcg, op):
    for n in V.SIZES_D:
        for run in V.layout_d(V.OPS[op][0], n):    # every class at every size (n = 1: one launch per class)
            _check(dc, dcg, op, run, "layout (d) n=%d" % n)


@pytest.mark.parametrize("op", OPS)
def test_divergent_lanes_e(dc, dcg, op):
    vec = V.layout_a(V.OPS[op][0])
    for pattern in V.PATTERNS_E:
        _check(dc, dcg, op, vec, "layout (e) pattern %#018x" % pattern, 1, pattern)
    _check(dc, dcg, op, V.layout_c(V.OPS[op][0]), "layout (c) divergent", 1, V.PATTERNS_E[0])   # equal operands, different operations, one wavefront


@pytest.mark.parametrize("op", OPS)
def test_generic_forms_on_the_device_pass_the_same_vectors(dc, dcg, op):
    assert dcg.dc_flags() == 7 and dc.dc_flags() == 0
    _check(dcg, dc, op, V.layout_a(V.OPS[op][0]), "generic build, layout (a)")


# ------------------------------------------------------------------ the product's kernels on edge-laden tables
def mm(a, b):
    return a * b * RINV % Q     # Montgomery product of residues


def _edge_values():
    vec = V.layout_a("fq")
    return [x for _, a, b in vec for x in (a, b)]


def _table(layout, n, k):
    """n Montgomery residues from the Fq edge pool: (a) neighbours differ, (c) runs of 64 equal values; k: which table of a set"""
    pool = _edge_values()
    off = 977 * k
    if layout == "a":
        return [pool[(off + i) % len(pool)] for i in range(n)]
    return [pool[(off + i // 64) % len(pool)] for i in range(n)]


def _arr(vals):
    return (ctypes.c_uint64 * (4 * len(vals))).from_buffer_copy(V.pack(vals))


def _ints(arr, n=None):
    raw = bytes(arr)
    n = len(raw) // 32 if n is None else n
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


def _py_eval(kind, T):
    n = len(T[0]); h = n // 2
    e0 = e2 = e3 = 0
    for i in range(h):
        p = []
        for t in T:
            x0, x1 = t[i], t[h + i]
            x2 = (2 * x1 - x0) % Q
            p.append((x0, x2, (x2 + x1 - x0) % Q))
        A, B = p[0], p[1]
        if kind == 0:
            e0 += mm(A[0], B[0]); e2 += mm(A[1], B[1])
        elif kind == 1:
            C = p[2]
            e0 += mm(mm(A[0], B[0]), C[0]); e2 += mm(mm(A[1], B[1]), C[1]); e3 += mm(mm(A[2], B[2]), C[2])
        else:
            C, D = p[2], p[3]
            e0 += mm(A[0], mm(B[0], C[0]) - D[0]); e2 += mm(A[1], mm(B[1], C[1]) - D[1]); e3 += mm(A[2], mm(B[2], C[2]) - D[2])
    return [e0 % Q, e2 % Q] + ([e3 % Q] if kind else [])


def _py_bind(t, r):
    h = len(t) // 2
    return [(t[i] + mm(r, t[h + i] - t[i])) % Q for i in range(h)]


def _r_values(seed):
    return [0, 1, Q - 1, random.Random(seed).randrange(Q)]      # Montgomery residues


@pytest.mark.parametrize("layout", ["a", "c"])
@pytest.mark.parametrize("ell", [1, 6, 13])
@pytest.mark.parametrize("kind,ntabs", [(0, 2), (1, 3), (2, 4)])
@_flags_device_errors
def test_sumcheck_kernels_on_edge_tables(ctx, orc, kind, ntabs, ell, layout):
    from spartan_amd import capi
    n = 1 << ell
    T = [_table(layout, n, k + 4 * kind) for k in range(ntabs)]
    nv = 2 if kind == 0 else 3
    tabs = [capi.Table.upload(ctx, _arr(t), n) for t in T]
    got = _ints(capi.sumcheck_eval(ctx, kind, tabs), nv)
    host = [_arr(t) for t in T] + [None] * (4 - ntabs)
    w = (ctypes.c_uint64 * 12)()
    orc.orc_sumcheck_eval(ctypes.c_int(kind), host[0], host[1], host[2], host[3], sz(n), w)
    want = _py_eval(kind, T)
    assert _ints(w, nv) == want, "oracle and Python differ"
    assert got == want, ("sumcheck_eval", kind, ell, layout)
    assert _ints(capi.heads(ctx, tabs)) == [t[0] for t in T]
    for t in tabs:
        t.free()
    for r in _r_values(ell):
        tabs = [capi.Table.upload(ctx, _arr(t), n) for t in T]
        B = [_py_bind(t, r) for t in T]
        if n >= 4:      # the fused call needs two entries left after the bind (sp_sumcheck_bind_eval refuses len < 4): at ell = 1 bind_top does the bind
            got = _ints(capi.sumcheck_bind_eval(ctx, kind, tabs, _arr([r])), nv)
            assert got == _py_eval(kind, B), ("sumcheck_bind_eval", kind, ell, layout, hex(r))
        else:
            capi.bind_top(ctx, tabs, _arr([r]))
        for t, b in zip(tabs, B):
            assert len(t) == n // 2 and _ints(t.download(n // 2)) == b, ("bound table", kind, ell, layout, hex(r))
        assert _ints(capi.heads(ctx, tabs)) == [b[0] for b in B]
        for t in tabs:
            t.free()


@pytest.mark.parametrize("layout", ["a", "c"])
@pytest.mark.parametrize("v", [6, 13])
@_flags_device_errors
def test_linear_kernels_on_edge_tables(ctx, orc, v, layout):
    """bind_top, dot, vecmat, evaluate and Table.eq with tables, vectors and points of evaluation from the edge pool (0, 1 and q - 1 as
    Montgomery residues among the coordinates of r), against Python and, where it has the entry point, the oracle"""
    from spartan_amd import capi
    n = 1 << v
    Z, W = _table(layout, n, 20), _table(layout, n, 21)
    tz, tw = capi.Table.upload(ctx, _arr(Z), n), capi.Table.upload(ctx, _arr(W), n)
    # dot
    want = sum(mm(a, b) for a, b in zip(Z, W)) % Q
    o = u64x4(); orc.orc_dot(_arr(Z), _arr(W), sz(n), o)
    assert _ints(o) == [want] and _ints(capi.dot(ctx, tz, tw, n)) == [want]
    # vecmat: out[j] = sum_i L[i] Z[i * cols + j]
    Ls = 1 << (v // 2); cols = n // Ls
    Lv = _table("a", Ls, 22)
    want = [sum(mm(Lv[i], Z[i * cols + j]) for i in range(Ls)) % Q for j in range(cols)]
    o = (ctypes.c_uint64 * (4 * cols))(); orc.orc_bound_vecmat(_arr(Z), sz(v), _arr(Lv), o)
    assert _ints(o) == want and _ints(capi.vecmat(ctx, _arr(Lv), Ls, tz)) == want
    # eq(r) and evaluate
    r = ([0, 1, Q - 1] + _table("a", v, 23))[:v]
    one = R % Q
    chi = [one]
    for rj in r:
        chi = [x for e in chi for x in (mm(e, (one - rj) % Q), mm(e, rj))]
    o = (ctypes.c_uint64 * (4 * n))(); orc.orc_eq_evals(_arr(r), sz(v), o)
    assert _ints(o) == chi, "oracle and Python differ"
    te = capi.Table.eq(ctx, _arr(r), v)
    assert _ints(te.download()) == chi
    te.free()
    assert _ints(capi.evaluate(ctx, tz, _arr(r), v)) == [sum(mm(a, b) for a, b in zip(Z, chi)) % Q]
    # bind_top at each edge r, down to one entry
    cur = [Z, W]
    for k in range(v):
        rk = _r_values(v)[k % 4]
        capi.bind_top(ctx, [tz, tw], _arr([rk]))
        cur = [_py_bind(t, rk) for t in cur]
        if k in (0, 1, v - 1):
            assert _ints(tz.download(len(cur[0]))) == cur[0] and _ints(tw.download(len(cur[1]))) == cur[1], ("bind_top", v, layout, k)
    assert _ints(capi.heads(ctx, [tz, tw])) == [cur[0][0], cur[1][0]]
    tz.free(); tw.free()
