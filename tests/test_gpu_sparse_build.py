"""R1CS matrices built on the device from caller-format entry lists (spartan_amd/csrc/sparse_build.hip: sp_sparse_from_entries,
sp_sparse_from_entries_dev) against the same matrix uploaded with sp_sparse_upload from entries that Python checked, shifted and converted,
and against the Python-integer model of tests/sparse_build_reference.py. Everything is compared EXACTLY: the products, the satisfiability
report, the entry-order lists, the stored entries, the status and the four report words wherever the failing entry sits in a wavefront or a
workgroup."""
import ctypes, os, random, re
import pytest
from tests.helpers import *
from tests import sparse_build_reference as sb
from tests import field_vectors as V

pytestmark = pytest.mark.gpu
u64 = ctypes.c_uint64
EDGE = [0, 1, Q - 1] + V.fq_special_operands()


def _block_size():
    src = open(os.path.join(ROOT, "spartan_amd", "csrc", "sparse_build.hip")).read()
    m = re.search(r"constexpr unsigned BUILD_BLOCK = (\d+);", src)
    assert m and "(n + BUILD_BLOCK - 1) / BUILD_BLOCK" in src and "gridDim" not in src   # one lane per element: no cap, no stride
    return int(m.group(1))


B = _block_size()
SIZES = sorted({0, 1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 4099, 65537})
# the caller's 37 x (100 + 1 + 7) padded to 64 x 256 with a shift of 28, and the smallest shape: two rows (one key bit)
G_WIDE = dict(row_limit=37, col_limit=108, col_split=100, col_shift=28, pad_count=0, pad_col=100, num_rows=64, num_cols=256)
G_TWO = dict(row_limit=2, col_limit=5, col_split=3, col_shift=1, pad_count=0, pad_col=3, num_rows=2, num_cols=8)


@pytest.fixture(scope="module")
def L():
    from spartan_amd import capi
    return capi.lib


class RawCtx:
    """the sp_ctx* of a prover context in the shape capi.Table takes it. The context is made through spartan_amd.prover, which loads the
    library's HIP runtime for the whole process: torch, imported later for the device buffers of the _dev form, then shares it."""
    def __init__(self, pctx):
        self.pctx, self.h = pctx, pctx.raw()


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import prover
    c = RawCtx(prover.Ctx(0))
    yield c
    c.pctx.close()


def _values(rng, n):
    """EDGE cycled through the even positions, random values on the odd ones"""
    return [EDGE[(k // 2) % len(EDGE)] if k % 2 == 0 else rng.getrandbits(300) % Q for k in range(n)]


def _entries(rng, n, g, kind):
    vals = _values(rng, n)
    edge_cols = [g["col_split"] - 1, g["col_split"], g["col_limit"] - 1, 0]
    if kind == "spread":      # the columns on both sides of the split and the last one, then anything
        return [(rng.randrange(g["row_limit"]), edge_cols[k % 4] if k % 3 == 0 else rng.randrange(g["col_limit"]), vals[k]) for k in range(n)]
    if kind == "one_row":
        return [(g["row_limit"] - 1, rng.randrange(g["col_limit"]), vals[k]) for k in range(n)]
    if kind == "one_col":     # a shifted column
        return [(rng.randrange(g["row_limit"]), g["col_split"], vals[k]) for k in range(n)]
    if kind == "repeat":      # three (row, col) pairs over and over
        pairs = [(0, g["col_split"] - 1), (g["row_limit"] - 1, g["col_limit"] - 1), (0, 0)]
        return [pairs[rng.randrange(3)] + (vals[k],) for k in range(n)]
    raise ValueError(kind)


def _arrays(entries):
    n = len(entries)
    rows = (u64 * max(n, 1))(*[e[0] for e in entries]); cols = (u64 * max(n, 1))(*[e[1] for e in entries])
    return rows, cols, b"".join(e[2].to_bytes(32, "little") for e in entries)


def _geom(g):
    return (u64(g["row_limit"]), u64(g["col_limit"]), u64(g["col_split"]), u64(g["col_shift"]), sz(g["pad_count"]), u64(g["pad_col"]), sz(g["num_rows"]),
            sz(g["num_cols"]))


def _from_host(L, ctx, entries, g):
    rows, cols, vals = _arrays(entries)
    h, rep = vp(0xdead), (u64 * 4)(7, 7, 7, 7)
    rc = L.sp_sparse_from_entries(ctx.h, rows, cols, vals, sz(len(entries)), *_geom(g), ctypes.byref(h), rep)
    return rc, h, [int(x) for x in rep]


def _from_dev(L, ctx, entries, g, offset=0):
    """the three arrays in one device allocation, each `offset` bytes past an 8-byte boundary"""
    import torch
    n = len(entries)
    rows, cols, vals = _arrays(entries)
    span = (8 * n + 15) & ~7
    blob = bytearray(2 * span + 32 * n + 16)
    o = [offset, span + offset, 2 * span + offset]
    blob[o[0]:o[0] + 8 * n] = bytes(rows)[:8 * n]; blob[o[1]:o[1] + 8 * n] = bytes(cols)[:8 * n]; blob[o[2]:o[2] + 32 * n] = vals
    t = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 8 == 0
    h, rep = vp(0xdead), (u64 * 4)(7, 7, 7, 7)
    rc = L.sp_sparse_from_entries_dev(ctx.h, vp(t.data_ptr() + o[0]), vp(t.data_ptr() + o[1]), vp(t.data_ptr() + o[2]), sz(n), *_geom(g),
                                      ctypes.byref(h), rep)
    return rc, h, [int(x) for x in rep]


def _upload(L, ctx, ent, g):
    n = len(ent)
    rows = (u64 * max(n, 1))(*[e[0] for e in ent]); cols = (u64 * max(n, 1))(*[e[1] for e in ent])
    h = vp()
    assert L.sp_sparse_upload(ctx.h, rows, cols, mont_bulk([e[2] for e in ent]) if n else (u64 * 4)(), sz(n), sz(g["num_rows"]), sz(g["num_cols"]),
                              ctypes.byref(h)) == 0
    return h


class Probe:
    """the vectors every handle of one comparison is asked about, uploaded once"""
    def __init__(self, ctx, rng, g, edge):
        from spartan_amd import capi
        nr, nc = g["num_rows"], g["num_cols"]
        pick = (lambda n: [EDGE[rng.randrange(len(EDGE))] for _ in range(n)]) if edge else (lambda n: [rng.getrandbits(300) % Q for _ in range(n)])
        self.z, self.tx, self.ty, self.w = pick(nc), pick(nr), pick(nc), pick(1)
        self.tz, self.ttx, self.tty = (capi.Table.upload(ctx, mont_bulk(v), len(v)) for v in (self.z, self.tx, self.ty))

    def free(self):
        for t in (self.tz, self.ttx, self.tty):
            t.free()


def _observe(L, ctx, h, g, n, pr):
    """everything the library says about a matrix, as plain integers"""
    from spartan_amd import capi
    nr, nc = g["num_rows"], g["num_cols"]
    out = {}
    o = vp()
    assert L.sp_sparse_mulvec(ctx.h, h, pr.tz.h, ctypes.byref(o)) == 0
    t = capi.Table(ctx, o); out["mulvec"] = from_mont_bulk(t.download(), nr); t.free()
    o = vp()
    assert L.sp_sparse_eval_table(ctx.h, (vp * 1)(h), mont_bulk(pr.w), sz(1), pr.ttx.h, ctypes.byref(o)) == 0
    t = capi.Table(ctx, o); out["eval_table"] = from_mont_bulk(t.download(), nc); t.free()
    o4 = u64x4()
    assert L.sp_sparse_evaluate(ctx.h, h, pr.ttx.h, pr.tty.h, o4) == 0
    out["evaluate"] = from_mont_limbs(o4)
    nv, first, rows = u64(), u64(), (u64 * nr)()
    for _ in range(2):    # the second call runs from the long-row plan the first one built
        assert L.sp_r1cs_check(ctx.h, h, h, h, pr.tz.h, ctypes.byref(nv), ctypes.byref(first), rows, sz(nr)) == 0
        out.setdefault("check", []).append((nv.value, first.value, list(rows[:nv.value])))
    N = n + 3             # zero-padded lists, as SNARK::encode asks for them
    dst = capi.Table.alloc(ctx, 3 * N)
    for which in (0, 1):
        ix = vp()
        assert L.sp_sparse_entry_index(ctx.h, h, ctypes.c_int(which), sz(N), ctypes.byref(ix)) == 0
        assert L.sp_table_from_index(ctx.h, ix, dst.h, sz(which * N)) == 0
        L.sp_index_free(ix)
    assert L.sp_sparse_entry_values(ctx.h, h, dst.h, sz(2 * N), sz(N)) == 0
    flat = from_mont_bulk(dst.download(), 3 * N); dst.free()
    out["entry_rows"], out["entry_cols"], out["entry_vals"] = flat[:N], flat[N:2 * N], flat[2 * N:]
    r32, c32, v = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))(), (u64 * (4 * max(n, 1)))()
    assert L.sp_sparse_download_entries(ctx.h, h, r32, c32, v) == 0
    out["entries"] = list(zip(list(r32)[:n], list(c32)[:n], from_mont_bulk(v, n)))
    return out


def _model(ent, g, pr):
    nr, nc = g["num_rows"], g["num_cols"]
    mv = sb.mulvec(ent, pr.z, nr)
    bad = [r for r in range(nr) if mv[r] * mv[r] % Q != mv[r]]
    chk = (len(bad), bad[0] if bad else sb.NONE, bad)
    pad = [0, 0, 0]
    return {"mulvec": mv, "eval_table": [pr.w[0] * x % Q for x in sb.eval_table(ent, pr.tx, nc)], "evaluate": sb.evaluate(ent, pr.tx, pr.ty),
            "check": [chk, chk], "entry_rows": [e[0] for e in ent] + pad, "entry_cols": [e[1] for e in ent] + pad,
            "entry_vals": [e[2] for e in ent] + pad, "entries": list(ent)}


def _compare(L, ctx, entries, g, seed, edge=False, dev=True, offset=1):
    st, rep, ent = sb.build(entries, g)
    assert st == sb.OK and not sb.invalid_arguments(len(entries), g)
    pr = Probe(ctx, random.Random(seed), g, edge)
    want = _model(ent, g, pr)
    handles = [("upload", _upload(L, ctx, ent, g))]
    rc, h, got_rep = _from_host(L, ctx, entries, g)
    assert rc == 0 and h.value not in (0, 0xdead) and got_rep == rep == [0, sb.NONE, 0, sb.NONE]
    handles.append(("from_entries", h))
    if dev:
        rc, h, got_rep = _from_dev(L, ctx, entries, g, offset)
        assert rc == 0 and got_rep == rep
        handles.append(("from_entries_dev", h))
    for name, h in handles:
        got = _observe(L, ctx, h, g, len(ent), pr)
        for key in want:
            assert got[key] == want[key], (name, key, len(entries))
        L.sp_sparse_free(h)
    pr.free()


@pytest.mark.parametrize("n", SIZES)
def test_every_size_on_the_wide_shape(L, ctx, n):
    _compare(L, ctx, _entries(random.Random(n), n, G_WIDE, "spread"), G_WIDE, seed=n, edge=(n % 2 == 1))


@pytest.mark.parametrize("n", [0, 1, 65, 4099])
def test_two_rows_is_one_key_bit(L, ctx, n):
    _compare(L, ctx, _entries(random.Random(7 + n), n, G_TWO, "spread"), G_TWO, seed=n, edge=True)


@pytest.mark.parametrize("kind,n", [("one_row", 33), ("one_row", 4099), ("one_col", 4099), ("repeat", 2 * B + 1), ("one_col", 64)])
def test_degenerate_key_distributions(L, ctx, kind, n):
    """every entry in one row (4099: beyond one lane's 32 entries and beyond one 1024-entry chunk of the check's long-row plan), every entry in
    one shifted column, three (row, col) pairs repeated: within a key the order is entry order, whatever the run length"""
    _compare(L, ctx, _entries(random.Random(n), n, G_WIDE, kind), G_WIDE, seed=n)


@pytest.mark.parametrize("nnz,pad", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_pad_entries(L, ctx, nnz, pad):
    """the explicit zero constraints of an instance with 0 or 1 constraints: entry e in [nnz, nnz + pad) is (e, pad_col, 0)"""
    g = dict(row_limit=1, col_limit=6, col_split=4, col_shift=0, pad_count=pad, pad_col=4, num_rows=4, num_cols=8)
    entries = [(0, 5, Q - 1)][:nnz]
    assert sb.build(entries, g)[2] == entries + [(e, 4, 0) for e in range(nnz, nnz + pad)]
    _compare(L, ctx, entries, g, seed=nnz + 2 * pad, edge=True)
    small = dict(g, num_rows=nnz + pad - 1)                      # the last pad entry would be row num_rows
    rc, h, rep = _from_host(L, ctx, entries, small)
    assert sb.invalid_arguments(nnz, small) and (rc, h.value, rep) == (sb.EINVAL, 0xdead, [7] * 4)


def _refused(L, ctx, entries, g, forms=("host",), offset=1):
    st, rep, ent = sb.build(entries, g)
    assert st in (sb.EINDEX, sb.ESCALAR) and ent is None
    for form in forms:
        rc, h, got = _from_host(L, ctx, entries, g) if form == "host" else _from_dev(L, ctx, entries, g, offset)
        assert (rc, h.value, got) == (st, None, rep), (form, rc, h.value, got, rep)
    return st, rep


def test_refusals_and_their_reports(L, ctx):
    rng = random.Random(5)
    g = G_WIDE
    good = _entries(rng, 300, g, "spread")
    put = lambda changes: [changes.get(k, e) for k, e in enumerate(good)]
    for k, bad in enumerate(sb.BAD_SCALARS):
        assert _refused(L, ctx, put({17 + k: (1, 1, bad)}), g, ("host", "dev")) == (sb.ESCALAR, [0, sb.NONE, 1, 17 + k])
    assert _refused(L, ctx, put({9: (g["row_limit"], 0, 1)}), g, ("host", "dev")) == (sb.EINDEX, [1, 9, 0, sb.NONE])
    assert _refused(L, ctx, put({9: (0, g["col_limit"], 1)}), g) == (sb.EINDEX, [1, 9, 0, sb.NONE])
    # 2^32 + a valid index is a bad index, not the valid one
    assert _refused(L, ctx, put({0: (2**32 + 3, 0, 1), 299: (0, 2**32 + 5, 1)}), g, ("host", "dev")) == (sb.EINDEX, [2, 0, 0, sb.NONE])
    assert _refused(L, ctx, put({5: (2**64 - 1, 2**64 - 1, 1)}), g) == (sb.EINDEX, [1, 5, 0, sb.NONE])
    # both faults in one entry: an index error only
    assert _refused(L, ctx, put({40: (g["row_limit"], 0, Q)}), g, ("host", "dev")) == (sb.EINDEX, [1, 40, 0, sb.NONE])
    # a bad scalar first, a bad index later, and the reverse: the lower one decides, both classes are reported
    assert _refused(L, ctx, put({70: (0, 0, Q + 1), 200: (99, 0, 1), 201: (0, 0, 2**255)}), g, ("host", "dev")) == (sb.ESCALAR, [1, 200, 2, 70])
    assert _refused(L, ctx, put({70: (0, 999, 1), 200: (0, 0, Q), 250: (99, 0, Q)}), g, ("host", "dev")) == (sb.EINDEX, [2, 70, 1, 200])
    # every entry bad, one class each
    assert _refused(L, ctx, [(99, 0, 1)] * 130, g)[1] == [130, 0, 0, sb.NONE]
    assert _refused(L, ctx, [(0, 0, 2**256 - 1)] * 130, g)[1] == [0, sb.NONE, 130, 0]
    _compare(L, ctx, good, g, seed=1, dev=False)                # the context after the refusals


def test_a_single_bad_entry_at_every_corner_of_the_launch(L, ctx):
    """lanes 0 and 63 of the first and the last wavefront of the first and the last workgroup, index and scalar faults in turn"""
    rng = random.Random(6)
    n = 4 * B
    good = _entries(rng, n, G_WIDE, "spread")
    corners = [0, 63, B - 64, B - 1, n - B, n - B + 63, n - 64, n - 1]
    assert len(set(corners)) == 8
    for k, p in enumerate(corners):
        for fault in ((G_WIDE["row_limit"], 0, 1), (0, 0, sb.BAD_SCALARS[k % 4])):
            entries = list(good); entries[p] = fault
            st, rep = _refused(L, ctx, entries, G_WIDE)
            assert rep in ([1, p, 0, sb.NONE], [0, sb.NONE, 1, p])
    both = list(good); both[corners[3]] = (0, 0, Q); both[corners[4]] = (0, 2**40, 1)      # the two classes in different workgroups
    assert _refused(L, ctx, both, G_WIDE, ("host", "dev")) == (sb.ESCALAR, [1, n - B, 1, B - 1])
    _compare(L, ctx, good, G_WIDE, seed=2, dev=True, offset=1)


def test_device_arrays_at_odd_offsets_and_arguments(L, ctx):
    rng = random.Random(8)
    ent = _entries(rng, 257, G_WIDE, "spread")
    for offset in (0, 1, 7):
        _compare(L, ctx, ent, G_WIDE, seed=offset, offset=offset)
    rows, cols, vals = _arrays(ent)
    h, rep = vp(0xdead), (u64 * 4)(7, 7, 7, 7)
    for change in (dict(num_rows=0), dict(row_limit=65), dict(col_limit=229), dict(pad_count=1, pad_col=256), dict(pad_count=64)):
        g = dict(G_WIDE, **change)
        assert sb.invalid_arguments(257, g)
        assert L.sp_sparse_from_entries(ctx.h, rows, cols, vals, sz(257), *_geom(g), ctypes.byref(h), rep) == sb.EINVAL
    assert L.sp_sparse_from_entries(ctx.h, None, cols, vals, sz(257), *_geom(G_WIDE), ctypes.byref(h), rep) == sb.EINVAL
    assert h.value == 0xdead and list(rep) == [7] * 4
    # an empty matrix may come with arrays or without
    for arrs in ((rows, cols, vals), (None, None, None)):
        assert L.sp_sparse_from_entries(ctx.h, *arrs, sz(0), *_geom(G_WIDE), ctypes.byref(h), rep) == 0 and list(rep) == [0, sb.NONE, 0, sb.NONE]
        L.sp_sparse_free(h)
