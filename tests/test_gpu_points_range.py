"""sp_msm_points_range / sp_msm_points_range_many and sp_points_from_uniform (spartan_amd/csrc/msm_var.hip): the multiplication over n
consecutive points of a resident set, byte for byte against the oracle's orc_pt_msm over the slice and against sp_msm_points on a set uploaded
from the slice; and a resident set made on the device from a generator stream's uniform bytes, against sp_gens_from_uniform, the oracle's
MultiCommitGens and sp_points_upload of the same encodings. Ranges sit on the window-sum kernel's block (256) — short of it, on it, past it,
starting off a block boundary, ending at the set's end — and either side of where the call's 32 n bytes of scalars leave the host-mapped page."""
import ctypes, hashlib, random
import pytest
from tests.helpers import *
from tests import msm_var_cases as M
from tests.test_gpu_msm_many import hmap_gen

pytestmark = pytest.mark.gpu
PAGE_N = hmap_gen() // 32      # the last n whose scalars are read from the host-mapped page; PAGE_N + 1 is staged on the device
assert PAGE_N == 704
COUNTS = [1, 64, 257, 705, 1026]
KINDS = ["uniform", "sparse", "small", "edge"]
SP_EINVAL = -1
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


def ranges_of(count):
    """the (off, n) of the issue that fit a set of `count` points, each once"""
    cand = [(0, count), (0, 1), (count - 1, 1), (0, 255), (0, 256), (0, 257), (1, 256), (count - 256, 256), (0, PAGE_N), (0, PAGE_N + 1)]
    return sorted({(o, n) for o, n in cand if o >= 0 and n >= 1 and o + n <= count})


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    c = capi.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    from spartan_amd import capi
    return capi.lib


class Points:
    def __init__(self, L, ctx, pts=None, uniform=None):
        self.L, self.ctx, self.h, self.comp = L, ctx, vp(), None
        if pts is not None:
            self.n = len(pts)
            self.rc = L.sp_points_upload(ctx.h, b"".join(pts), sz(self.n), ctypes.byref(self.h))
        else:
            self.n = len(uniform) // 64
            out = (ctypes.c_uint8 * (32 * self.n))()
            self.rc = L.sp_points_from_uniform(ctx.h, uniform, sz(self.n), out, ctypes.byref(self.h))
            self.comp = bytes(out)

    def range(self, off, scalars):
        out = (ctypes.c_uint8 * 32)(*([0xA5] * 32))
        rc = self.L.sp_msm_points_range(self.ctx.h, self.h, sz(off), sz(len(scalars)), mont_array(scalars), out)
        return rc, bytes(out)

    def range_many(self, off, vecs):
        K, n = len(vecs), len(vecs[0])
        out = (ctypes.c_uint8 * (32 * K))(*([0xA5] * (32 * K)))
        rc = self.L.sp_msm_points_range_many(self.ctx.h, self.h, sz(off), sz(n), mont_array([s for v in vecs for s in v]), sz(K), out)
        return rc, [bytes(out[32 * k:32 * k + 32]) for k in range(K)]

    def whole(self, scalars):
        out = (ctypes.c_uint8 * 32)(*([0xA5] * 32))
        rc = self.L.sp_msm_points(self.ctx.h, self.h, mont_array(scalars), sz(len(scalars)), out)
        return rc, bytes(out)

    def free(self):
        if self.h:
            self.L.sp_points_free(self.h); self.h = vp()


@pytest.fixture(scope="module")
def big(L, ctx, orc):
    """the 1026-point set several tests address by range"""
    pts = M.points(orc, 1026)
    ps = Points(L, ctx, pts)
    assert ps.rc == 0
    yield pts, ps
    ps.free()


@pytest.mark.parametrize("count", COUNTS)
def test_range_matches_the_oracle_and_a_set_of_the_slice(L, ctx, orc, count):
    pts = M.points(orc, count)
    ps = Points(L, ctx, pts)
    assert ps.rc == 0 and L.sp_points_count(ps.h) == count
    try:
        for off, n in ranges_of(count):
            sl = Points(L, ctx, pts[off:off + n])
            assert sl.rc == 0
            try:
                for kind in KINDS:
                    rng = random.Random(100000 * count + 100 * off + n + KINDS.index(kind))
                    S = rand_scalars(rng, n, kind)
                    rc, got = ps.range(off, S)
                    assert rc == 0, (count, off, n, kind, rc)
                    assert got == M.oracle_msm(orc, pts[off:off + n], S), (count, off, n, kind)
                    assert (0, got) == sl.whole(S), (count, off, n, kind)
            finally:
                sl.free()
    finally:
        ps.free()


@pytest.mark.parametrize("off,n", [(1, 256), (0, 257)])
def test_range_many_is_k_single_calls(big, orc, off, n):
    pts, ps = big
    for K in (1, 2, 3, 5):
        rng = random.Random(1000 * K + off + n)
        vecs = [rand_scalars(rng, n, KINDS[(k + K) % 4]) for k in range(K)]
        rc, got = ps.range_many(off, vecs)
        assert rc == 0, (K, rc)
        for k, S in enumerate(vecs):
            assert (0, got[k]) == ps.range(off, S), (K, k)
            assert got[k] == M.oracle_msm(orc, pts[off:off + n], S), (K, k)


@pytest.mark.parametrize("n,off", [(64, 3), (257, 300)])
def test_named_cases_inside_a_larger_set(L, ctx, orc, n, off):
    """the identity, repeats and mutual negatives as a range of a set that has other points before and after it"""
    rng = random.Random(n)
    pad = M.points(orc, 700, seed=5)
    for name, pts, S in M.named_cases(orc, rng, n):
        ps = Points(L, ctx, pad[:off] + list(pts) + pad[off:off + 40])
        try:
            assert ps.rc == 0, (name, ps.rc)
            rc, got = ps.range(off, S)
            assert rc == 0, (name, rc)
            assert got == M.oracle_msm(orc, pts, S), (name, n)
            if name in ("all_zero", "only_a_pair_of_negatives"):
                assert got == M.IDENTITY, name
        finally:
            ps.free()


def test_error_returns(L, ctx, big, orc):
    pts, ps = big
    out = (ctypes.c_uint8 * 32)()
    S = mont_array(list(range(1, 1028)))
    call = lambda off, n: L.sp_msm_points_range(ctx.h, ps.h, sz(off), sz(n), S, out)
    assert call(0, 0) == SP_EINVAL
    assert call(0, 1027) == SP_EINVAL and call(1, 1026) == SP_EINVAL and call(1026, 1) == SP_EINVAL      # off + n = count + 1
    assert call(2**64 - 1, 2) == SP_EINVAL                                                              # off + n wraps
    assert L.sp_msm_points_range(None, ps.h, sz(0), sz(1), S, out) == SP_EINVAL
    assert L.sp_msm_points_range(ctx.h, None, sz(0), sz(1), S, out) == SP_EINVAL
    assert L.sp_msm_points_range(ctx.h, ps.h, sz(0), sz(1), None, out) == SP_EINVAL
    assert L.sp_msm_points_range(ctx.h, ps.h, sz(0), sz(1), S, None) == SP_EINVAL
    outs = (ctypes.c_uint8 * 64)()
    many = lambda off, n, K: L.sp_msm_points_range_many(ctx.h, ps.h, sz(off), sz(n), S, sz(K), outs)
    assert many(0, 0, 2) == SP_EINVAL and many(0, 2, 0) == SP_EINVAL and many(1025, 2, 2) == SP_EINVAL and many(0, 2, 257) == SP_EINVAL
    # the whole-set calls keep their contract: a scalar count that is not the set's size
    assert L.sp_msm_points(ctx.h, ps.h, S, sz(1025), out) == SP_EINVAL and L.sp_msm_points(ctx.h, ps.h, S, sz(1027), out) == SP_EINVAL
    assert L.sp_msm_points(ctx.h, ps.h, S, sz(0), out) == SP_EINVAL
    assert L.sp_msm_points_many(ctx.h, ps.h, S, sz(513), sz(2), outs) == SP_EINVAL
    assert L.sp_points_table_bytes(None) == 0
    # and the set still answers
    assert call(1025, 1) == 0 and bytes(out) == M.oracle_msm(orc, pts[1025:], [1])


def test_a_set_is_reused_over_two_ranges(big, orc):
    pts, ps = big
    rng = random.Random(17)
    a, b = (1, 256), (300, 705)
    Sa, Sb = rand_scalars(rng, a[1], "edge"), rand_scalars(rng, b[1])
    first = (ps.range(a[0], Sa), ps.range(b[0], Sb))
    assert first == ((0, M.oracle_msm(orc, pts[1:257], Sa)), (0, M.oracle_msm(orc, pts[300:1005], Sb)))
    for _ in range(3):
        assert (ps.range(a[0], Sa), ps.range(b[0], Sb)) == first


@pytest.mark.parametrize("n", [1, 5, 64, 65, 257, 1026])
def test_points_from_uniform(L, ctx, orc, n):
    from spartan_amd import capi
    uniform = hashlib.shake_256(b"gens_r1cs_sat" + BASEPOINT).digest(64 * n)
    ps = Points(L, ctx, uniform=uniform)
    assert ps.rc == 0 and L.sp_points_count(ps.h) == n and L.sp_points_table_bytes(ps.h) == 65536 * n
    up = None
    try:
        ctx.set_option("msm.wbits", 8)         # the comparison set's fixed-base tables: narrow, they are not used here
        try:
            g = capi.Gens(ctx, uniform=uniform)
        finally:
            ctx.set_option("msm.wbits", 0)
        try:
            assert ps.comp == g.compressed
        finally:
            g.free()
        if n >= 2:
            assert ps.comp == gens_bytes(orc, n - 1)           # MultiCommitGens::new(n - 1, label): n - 1 points G, then h
        else:
            assert ps.comp == gens_bytes(orc, 1)[:32]
        pts = [ps.comp[32 * i:32 * i + 32] for i in range(n)]
        up = Points(L, ctx, pts)
        assert up.rc == 0
        for kind in KINDS:
            S = rand_scalars(random.Random(10 * n + KINDS.index(kind)), n, kind)
            want = M.oracle_msm(orc, pts, S)
            assert ps.whole(S) == (0, want), (n, kind)
            assert up.whole(S) == (0, want), (n, kind)
        if n > 2:   # a prefix and a suffix of the stream, as the verifier addresses it
            S = rand_scalars(random.Random(n), n - 2)
            assert ps.range(0, S) == (0, M.oracle_msm(orc, pts[:n - 2], S))
            assert ps.range(2, S) == (0, M.oracle_msm(orc, pts[2:], S))
        h = vp()
        assert L.sp_points_from_uniform(ctx.h, uniform, sz(0), None, ctypes.byref(h)) == SP_EINVAL
        assert L.sp_points_from_uniform(ctx.h, None, sz(n), None, ctypes.byref(h)) == SP_EINVAL and not h
    finally:
        ps.free()
        if up:
            up.free()
