"""sp_sparse_evaluate_many_begin (spartan_amd/csrc/sparse_many.hip) through capi.lib: R1CSInstance::evaluate of up to four matrices at K points
in one pass, from half tables only. Every result is compared EXACTLY with two yardsticks: the Python-integer model
(tests/eval_many_reference.py) and the existing sp_eq_expand x 2 + sp_sparse_evaluate run for that proof alone. Shapes are the smallest at
which each path can go wrong (the lists of eval_many_reference; tests/test_eval_many_reference.py holds them to the dispatch)."""
import ctypes, random
import pytest
from tests.helpers import *
from tests import eval_many_reference as E
from tests import field_vectors as V

pytestmark = pytest.mark.gpu
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)
EDGES = V.fq_special_operands()        # 0, 1, R, R^2, q - 1, q - 2, 2^252 +- .., (q - 1) / 2, 0xffffffff in each word: raw residues


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    c = capi.Ctx(0)
    yield c
    c.close()


def raw(vals):
    """raw residues -> ctypes uint64 limbs, as they are"""
    n = max(len(vals), 1)
    return (ctypes.c_uint64 * (4 * n)).from_buffer_copy(b"".join(x.to_bytes(32, "little") for x in vals) + bytes(32 * (n - len(vals))))


def ints(buf, n):
    b = bytes(buf)
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(n)]


def scalar(rng, p_edge=0.35):
    return EDGES[rng.randrange(len(EDGES))] if rng.random() < p_edge else rng.randrange(Q)


def points(rng, K, ell):
    """K challenge vectors: the first three all zeros, all ones, all q - 1 (where K has room), the rest edge values mixed with random ones"""
    fixed = [[0] * ell, [E.ONE] * ell, [Q - 1] * ell]
    return [fixed[k] if k < 3 and K > 3 else [scalar(rng) for _ in range(ell)] for k in range(K)]


def entries(rng, nnz, nr, nc, kind="random"):
    if kind == "one_row":
        r = rng.randrange(nr)
        return [(r, rng.randrange(nc), scalar(rng)) for _ in range(nnz)]
    if kind == "one_col":
        c = rng.randrange(nc)
        return [(rng.randrange(nr), c, scalar(rng)) for _ in range(nnz)]
    if kind == "repeated":
        pairs = [(rng.randrange(nr), rng.randrange(nc)) for _ in range(3)]
        return [(*pairs[i % 3], scalar(rng)) for i in range(nnz)]
    out = [(rng.randrange(nr), rng.randrange(nc), scalar(rng)) for _ in range(nnz)]
    if nnz >= 2:       # the corners of the shape: the last row and the last column are read
        out[0] = (nr - 1, nc - 1, out[0][2]); out[-1] = (0, 0, out[-1][2])
    return out


class Mats:
    """matrices uploaded to the device, freed on exit"""
    def __init__(self, ctx, mats, nr, nc):
        from spartan_amd import capi
        self.L, self.ctx, self.mats, self.nr, self.nc, self.hs = capi.lib, ctx, mats, nr, nc, []
        for M in mats:
            n = len(M)
            h = vp()
            rows = (ctypes.c_uint64 * max(n, 1))(*[e[0] for e in M]); cols = (ctypes.c_uint64 * max(n, 1))(*[e[1] for e in M])
            assert self.L.sp_sparse_upload(ctx.h, rows, cols, raw([e[2] for e in M]), sz(n), sz(nr), sz(nc), ctypes.byref(h)) == 0
            self.hs.append(h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for h in self.hs:
            self.L.sp_sparse_free(h)

    def begin(self, rxs, rys, ell_x, ell_y):
        K = len(rxs)
        job = vp()
        rc = self.L.sp_sparse_evaluate_many_begin(self.ctx.h, (vp * len(self.hs))(*self.hs), sz(len(self.hs)), raw([x for r in rxs for x in r]), sz(ell_x),
                                                  raw([y for r in rys for y in r]), sz(ell_y), sz(K), ctypes.byref(job))
        assert rc == 0, rc
        return job, K

    def wait(self, job):
        h, K = job
        n = len(self.hs) * K
        out = (ctypes.c_uint8 * (32 * n))()
        assert self.L.sp_job_wait(h, out) == 0
        v = ints(out, n)
        return [v[k * len(self.hs):(k + 1) * len(self.hs)] for k in range(K)]     # proof-major: out[k * count + m]

    def many(self, rxs, rys, ell_x, ell_y):
        return self.wait(self.begin(rxs, rys, ell_x, ell_y))

    def single(self, rx, ry):
        """the existing path for one proof: sp_eq_expand x 2, then sp_sparse_evaluate per matrix"""
        tx, ty = vp(), vp()
        assert self.L.sp_eq_expand(self.ctx.h, raw(rx), sz(len(rx)), ctypes.byref(tx)) == 0
        assert self.L.sp_eq_expand(self.ctx.h, raw(ry), sz(len(ry)), ctypes.byref(ty)) == 0
        out = []
        for h in self.hs:
            o4 = (ctypes.c_uint64 * 4)()
            assert self.L.sp_sparse_evaluate(self.ctx.h, h, tx, ty, o4) == 0
            out.append(ints(o4, 1)[0])
        self.L.sp_table_free(tx); self.L.sp_table_free(ty)
        return out

    def check(self, rxs, rys, what):
        ell_x, ell_y = len(rxs[0]), len(rys[0])
        got = self.many(rxs, rys, ell_x, ell_y)
        model = E.evaluate_many(self.mats, rxs, rys)
        assert got == model, (what, [k for k in range(len(rxs)) if got[k] != model[k]][:4])
        alone = [self.single(rx, ry) for rx, ry in zip(rxs, rys)]
        assert got == alone, (what, [k for k in range(len(rxs)) if got[k] != alone[k]][:4])
        assert all(x < Q for row in got for x in row)
        return got


COUNTS = (1, 3, 4)


@pytest.mark.parametrize("ell", E.ELLS, ids=lambda e: "%dx%d" % e)
def test_every_k_at_every_split(ctx, ell):
    """K over every padding Kp and both sides of it, at every split of the two points; count and the matrices' sizes rotate with K so that
    every count meets every Kp class, with unequal nnz and an empty matrix beside a full one"""
    ell_x, ell_y = ell
    rng = random.Random(1000 * ell_x + ell_y)
    full_r, full_c = 1 << ell_x, 1 << ell_y
    for i, K in enumerate(E.KS):
        count = COUNTS[(i + ell_x) % 3]
        nr, nc = (full_r, full_c) if i % 2 == 0 else (max(1, full_r - 1), max(1, full_c - 1))       # also shapes that are no power of two
        sizes = [E.NNZS[(i + m + ell_y) % len(E.NNZS)] for m in range(count)]
        if count > 1:
            sizes[1] = 0                                                                             # an empty matrix beside a full one
        mats = [entries(rng, n, nr, nc) for n in sizes]
        with Mats(ctx, mats, nr, nc) as M:
            M.check(points(rng, K, ell_x), points(rng, K, ell_y), (ell, K, count, sizes))


@pytest.mark.parametrize("K", (1, 3, 64))
def test_every_nnz_boundary(ctx, K):
    """0, 1 and the entries around the first block boundary as the only matrix of a call, at the small and at the large split"""
    rng = random.Random(2000 + K)
    for ell_x, ell_y in ((2, 3), (13, 14)):
        for nnz in E.NNZS:
            with Mats(ctx, [entries(rng, nnz, 1 << ell_x, 1 << ell_y)], 1 << ell_x, 1 << ell_y) as M:
                got = M.check(points(rng, K, ell_x), points(rng, K, ell_y), (K, ell_x, ell_y, nnz))
                if nnz == 0:
                    assert got == [[0]] * K


@pytest.mark.parametrize("K", (3, 64))
def test_the_cap_of_the_partials_grid_and_past_it(ctx, K):
    """a matrix whose grid just reaches the cap read from the source, and one whose first block takes a second grid-stride pass, next to a
    small one (its blocks past the first few have no entry and must write zeros)"""
    rng = random.Random(3000 + K)
    at, past = E.nnz_at_cap(K)
    assert E.blocks(at, K) == E.partials_cap() and E.blocks(at - 1, K) < E.partials_cap()
    ell_x, ell_y = 8, 9
    for nnz in (at, past):
        with Mats(ctx, [entries(rng, 7, 1 << ell_x, 1 << ell_y), entries(rng, nnz, 1 << ell_x, 1 << ell_y)], 1 << ell_x, 1 << ell_y) as M:
            M.check(points(rng, K, ell_x), points(rng, K, ell_y), (K, nnz))


@pytest.mark.parametrize("kind", ("one_row", "one_col", "repeated"))
def test_special_matrices(ctx, kind):
    rng = random.Random({"one_row": 4001, "one_col": 4002, "repeated": 4003}[kind])
    for (ell_x, ell_y), K in (((3, 5), 5), ((13, 14), 33)):
        mats = [entries(rng, 300, 1 << ell_x, 1 << ell_y, kind), entries(rng, 40, 1 << ell_x, 1 << ell_y), entries(rng, 257, 1 << ell_x, 1 << ell_y, kind)]
        with Mats(ctx, mats, 1 << ell_x, 1 << ell_y) as M:
            M.check(points(rng, K, ell_x), points(rng, K, ell_y), (kind, ell_x, ell_y, K))


def test_all_edge_values(ctx):
    """values and challenges from the edge set alone: zero, one, q - 1 and the carry edges in every factor"""
    rng = random.Random(5)
    ell_x, ell_y, K = 8, 9, 8
    mats = [[(rng.randrange(1 << ell_x), rng.randrange(1 << ell_y), EDGES[i % len(EDGES)]) for i in range(400)] for _ in range(3)]
    rxs = [[EDGES[(k + 3 * j) % len(EDGES)] for j in range(ell_x)] for k in range(K)]
    rys = [[EDGES[(5 * k + j + 1) % len(EDGES)] for j in range(ell_y)] for k in range(K)]
    with Mats(ctx, mats, 1 << ell_x, 1 << ell_y) as M:
        M.check(rxs, rys, "edges")


def test_refused_arguments_return_einval_and_the_context_still_evaluates(ctx):
    rng = random.Random(6)
    ell_x, ell_y, K = 2, 3, 3
    nr, nc = 1 << ell_x, 1 << ell_y
    with Mats(ctx, [entries(rng, 9, nr, nc), entries(rng, 5, nr, nc)], nr, nc) as M, Mats(ctx, [entries(rng, 4, nr + 1, nc)], nr + 1, nc) as tall, \
            Mats(ctx, [entries(rng, 4, nr, nc + 1)], nr, nc + 1) as wide:
        L = M.L
        rxs, rys = points(rng, K, ell_x), points(rng, K, ell_y)
        rx, ry = raw([x for r in rxs for x in r]), raw([y for r in rys for y in r])
        big = raw([0] * (33 * 65))
        hs = (vp * 2)(*M.hs)
        job = vp()
        def call(c=ctx.h, ms=hs, count=2, x=rx, ex=ell_x, y=ry, ey=ell_y, k=K, out=ctypes.byref(job)):
            return L.sp_sparse_evaluate_many_begin(c, ms, sz(count), x, sz(ex), y, sz(ey), sz(k), out)
        refused = {
            "null context": call(c=None), "null matrix list": call(ms=None), "null rx": call(x=None), "null ry": call(y=None), "null out": call(out=None),
            "count = 0": call(count=0), "count = 5": call(ms=(vp * 5)(*([M.hs[0]] * 5)), count=5),
            "K = 0": call(k=0), "K = 65": call(x=big, y=big, k=65),
            "ell_x = 0": call(ex=0), "ell_x = 33": call(x=big, ex=33), "ell_y = 0": call(ey=0), "ell_y = 33": call(y=big, ey=33),
            "a null matrix": call(ms=(vp * 2)(M.hs[0], None)),
            "num_rows > 2^ell_x": call(ms=(vp * 2)(M.hs[0], tall.hs[0])), "num_cols > 2^ell_y": call(ms=(vp * 2)(wide.hs[0], M.hs[1])),
        }
        assert refused == {k: -1 for k in refused}, refused                 # SP_EINVAL
        assert not job
        M.check(rxs, rys, "after the refusals")
        # the taller and the wider matrix are fine once the points have a variable more
        tall.check(points(rng, K, ell_x + 1), rys, "tall")
        wide.check(rxs, points(rng, K, ell_y + 1), "wide")


def test_two_jobs_begun_back_to_back_and_waited_for_in_the_other_order(ctx):
    rng = random.Random(7)
    a_ell, b_ell = (8, 9), (3, 5)
    with Mats(ctx, [entries(rng, 600, 1 << 8, 1 << 9) for _ in range(3)], 1 << 8, 1 << 9) as A, Mats(ctx, [entries(rng, 90, 1 << 3, 1 << 5)], 1 << 3, 1 << 5) as B:
        ax, ay = points(rng, 16, a_ell[0]), points(rng, 16, a_ell[1])
        bx, by = points(rng, 5, b_ell[0]), points(rng, 5, b_ell[1])
        ja = A.begin(ax, ay, *a_ell)
        jb = B.begin(bx, by, *b_ell)
        got_b = B.wait(jb)
        got_a = A.wait(ja)
        assert got_a == E.evaluate_many(A.mats, ax, ay)
        assert got_b == E.evaluate_many(B.mats, bx, by)
        assert got_a == [A.single(x, y) for x, y in zip(ax, ay)]
