"""sp_msm_var_many / sp_msm_points_many (spartan_amd/csrc/msm_var.hip): K variable-base multi-scalar multiplications of one size in one
launch chain and one round trip, every one of them byte for byte against the oracle's orc_pt_msm (M.oracle_msm). Sizes sit on the kernels'
edges (a wavefront, a window-sum block, more than one block), batch sizes 1, 2, 3, 5 and the wide, short batch of a full SNARK batch at 2^10
(n = 32, K = 64); both sides of the size at which the inputs leave the host-mapped page (read from internal.hpp); cross-talk between
neighbours of a batch; an undecodable point fails its own multiplication only; argument checks, the profile record and the trip count."""
import ctypes, os, random, re
import pytest
from tests.helpers import *
from tests import msm_var_cases as M

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
BATCHES = [1, 2, 3, 5]
KINDS = ["uniform", "sparse", "small", "edge"]
SP_OK, SP_EINVAL, SP_EPOINT = 0, -1, -4
MAX_N = 65536
_HDR = open(os.path.join(ROOT, "include", "spartan_hip.h")).read()
MAX_K = int(re.search(r"#define SP_MSM_MANY_MAX_K (\d+)u", _HDR).group(1))
MAX_TERMS = 1 << int(re.search(r"#define SP_MSM_MANY_MAX_TERMS \(1u << (\d+)\)", _HDR).group(1))
assert (MAX_K, MAX_TERMS) == (256, 1 << 20)            # the caps the issue names


def hmap_gen():
    """bytes of kernel input that go through the host-mapped page (internal.hpp: HMAP_GEN = HMAP_IN - EQ_SLOTS * EQ_SLOT_BYTES)"""
    src = open(os.path.join(ROOT, "spartan_amd", "csrc", "internal.hpp")).read()
    val = lambda name: int(re.search(r"\b%s = (\d+)" % name, src).group(1))
    assert re.search(r"HMAP_GEN = HMAP_IN - EQ_SLOTS \* EQ_SLOT_BYTES", src)
    return val("HMAP_IN") - val("EQ_SLOTS") * val("EQ_SLOT_BYTES")


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


def var_many(L, ctx, batch):
    """batch: [(points, scalars)] of one size -> (rc, [status], [32 bytes])"""
    K, n = len(batch), len(batch[0][0])
    pts = b"".join(b"".join(p) for p, _ in batch)
    S = mont_array([s for _, sc in batch for s in sc])
    out = (ctypes.c_uint8 * (32 * K))(*([0xA5] * (32 * K)))
    st = (ctypes.c_int32 * K)(*([77] * K))
    rc = L.sp_msm_var_many(ctx.h, pts, S, sz(n), sz(K), out, st)
    return rc, list(st), [bytes(out[32 * k:32 * k + 32]) for k in range(K)]


def var_one(L, ctx, pts, scalars):
    out = (ctypes.c_uint8 * 32)()
    rc = L.sp_msm_var(ctx.h, b"".join(pts), mont_array(scalars), sz(len(pts)), out)
    return rc, bytes(out)


class Points:
    def __init__(self, L, ctx, pts):
        self.L, self.ctx, self.n, self.h = L, ctx, len(pts), vp()
        assert L.sp_points_upload(ctx.h, b"".join(pts), sz(len(pts)), ctypes.byref(self.h)) == 0

    def many(self, vecs):
        K = len(vecs)
        out = (ctypes.c_uint8 * (32 * K))(*([0xA5] * (32 * K)))
        rc = self.L.sp_msm_points_many(self.ctx.h, self.h, mont_array([s for v in vecs for s in v]), sz(self.n), sz(K), out)
        return rc, [bytes(out[32 * k:32 * k + 32]) for k in range(K)]

    def one(self, scalars):
        out = (ctypes.c_uint8 * 32)()
        rc = self.L.sp_msm_points(self.ctx.h, self.h, mont_array(scalars), sz(self.n), out)
        return rc, bytes(out)

    def free(self):
        if self.h:
            self.L.sp_points_free(self.h); self.h = vp()


def make_batch(orc, n, K, seed):
    """K multiplications of n points each: their own points (K slices of one seeded stream) and scalar kinds in rotation"""
    rng = random.Random(seed)
    allp = M.points(orc, n * K, seed=11)
    return [(allp[k * n:(k + 1) * n], rand_scalars(rng, n, KINDS[(k + seed) % 4])) for k in range(K)]


_WANT = {}


def want(orc, pts, scalars):
    """the oracle's sum, computed once per input"""
    key = (b"".join(pts), tuple(scalars))
    if key not in _WANT:
        _WANT[key] = M.oracle_msm(orc, pts, scalars)
    return _WANT[key]


@pytest.mark.parametrize("n", SIZES)
def test_var_many_matches_the_oracle(L, ctx, orc, n):
    for K in BATCHES:
        for rot in range(4):      # the four kinds of scalars in rotation over the members: every member position sees every kind
            batch = make_batch(orc, n, K, rot)
            rc, st, got = var_many(L, ctx, batch)
            assert rc == SP_OK and st == [SP_OK] * K, (n, K, rc, st)
            for k, (p, s) in enumerate(batch):
                assert got[k] == want(orc, p, s), (n, K, k)


@pytest.mark.parametrize("n", SIZES)
def test_points_many_matches_the_oracle(L, ctx, orc, n):
    pts = M.points(orc, n)
    ps = Points(L, ctx, pts)
    try:
        for K in BATCHES:
            for rot in range(4):
                rng = random.Random(100 * n + 10 * K + rot)
                vecs = [rand_scalars(rng, n, KINDS[(k + rot) % 4]) for k in range(K)]
                rc, got = ps.many(vecs)
                assert rc == SP_OK, (n, K, rc)
                for k, v in enumerate(vecs):
                    assert got[k] == want(orc, pts, v), (n, K, k)
    finally:
        ps.free()


def test_the_wide_short_batch_of_64_proofs_at_2_10(L, ctx, orc):
    n, K = 32, 64
    batch = make_batch(orc, n, K, 5)
    rc, st, got = var_many(L, ctx, batch)
    assert rc == SP_OK and st == [SP_OK] * K
    assert got == [want(orc, p, s) for p, s in batch]
    pts = M.points(orc, n)
    ps = Points(L, ctx, pts)
    try:
        rc, got = ps.many([s for _, s in batch])
        assert rc == SP_OK and got == [want(orc, pts, s) for _, s in batch]
    finally:
        ps.free()


def test_both_sides_of_the_host_page_boundary(L, ctx, orc):
    """inputs of up to HMAP_GEN bytes are read from the host-mapped page, larger ones are copied to the device first: sp_msm_var_many stages
    64 n K bytes (encodings and scalars), sp_msm_points_many 32 n K (scalars)"""
    G = hmap_gen()
    assert G % 64 == 0
    shapes = [(G // 64, 1), (G // 64 + 1, 1), (32, G // (64 * 32)), (32, G // (64 * 32) + 1)]
    assert all((64 * n * K <= G) == (i % 2 == 0) for i, (n, K) in enumerate(shapes))
    for n, K in shapes:
        batch = make_batch(orc, n, K, n)
        rc, st, got = var_many(L, ctx, batch)
        assert rc == SP_OK and st == [SP_OK] * K, (n, K)
        assert got == [want(orc, p, s) for p, s in batch], (n, K)
    pshapes = [(G // 32, 1), (G // 32 + 1, 1), (32, G // (32 * 32)), (32, G // (32 * 32) + 1)]
    assert all((32 * n * K <= G) == (i % 2 == 0) for i, (n, K) in enumerate(pshapes))
    for n, K in pshapes:
        pts = M.points(orc, n)
        ps = Points(L, ctx, pts)
        try:
            rng = random.Random(n * K)
            vecs = [rand_scalars(rng, n, KINDS[k % 4]) for k in range(K)]
            rc, got = ps.many(vecs)
            assert rc == SP_OK and got == [want(orc, pts, v) for v in vecs], (n, K)
        finally:
            ps.free()


@pytest.mark.parametrize("n", [64, 257])
def test_no_cross_talk_between_the_multiplications_of_a_batch(L, ctx, orc, n):
    """all-zero scalars, identity points, a pair of negatives and repeated points, each between two random multiplications; the batch in
    reverse order gives the reversed results"""
    rng = random.Random(n)
    named = {name: (p, s) for name, p, s in M.named_cases(orc, rng, n)}
    picked = ["all_zero", "identity_among_inputs", "only_a_pair_of_negatives", "negatives_adjacent", "one_point_repeated"]
    fill = make_batch(orc, n, len(picked) + 1, 9)
    batch = [fill[0]]
    for i, name in enumerate(picked):
        batch += [named[name], fill[i + 1]]
    rc, st, got = var_many(L, ctx, batch)
    assert rc == SP_OK and st == [SP_OK] * len(batch)
    expect = [want(orc, p, s) for p, s in batch]
    assert got == expect
    assert got[1] == M.IDENTITY and got[5] == M.IDENTITY            # all-zero scalars; a pair of negatives under one scalar
    rc, st, rev = var_many(L, ctx, batch[::-1])
    assert rc == SP_OK and st == [SP_OK] * len(batch) and rev == expect[::-1]
    # the resident set: one of the named point sets under the named and the random scalar vectors in turn
    for name in ("identity_among_inputs", "only_a_pair_of_negatives", "one_point_repeated"):
        pts = named[name][0]
        ps = Points(L, ctx, pts)
        try:
            vecs = [fill[0][1], [0] * n, named[name][1], fill[1][1], [Q - 1] * n, fill[2][1]]
            rc, got = ps.many(vecs)
            exp = [want(orc, pts, v) for v in vecs]
            assert rc == SP_OK and got == exp, name
            assert got[1] == M.IDENTITY
            rc, rev = ps.many(vecs[::-1])
            assert rc == SP_OK and rev == exp[::-1], name
        finally:
            ps.free()


@pytest.mark.parametrize("n", [65, 257])
def test_an_undecodable_point_fails_its_own_multiplication_only(L, ctx, orc, n):
    from tests.test_oracle_pins import RFC_BAD
    K = 5
    good = make_batch(orc, n, K, 3)
    expect = [want(orc, p, s) for p, s in good]
    i = 0
    for k in (0, K // 2, K - 1):
        for where in (0, n - 1):
            batch = [(list(p), s) for p, s in good]
            batch[k][0][where] = bytes.fromhex(RFC_BAD[i % len(RFC_BAD)]); i += 1
            rc, st, got = var_many(L, ctx, batch)
            assert rc == SP_OK, (k, where, rc)
            assert st == [SP_EPOINT if j == k else SP_OK for j in range(K)], (k, where, st)
            assert [g for j, g in enumerate(got) if j != k] == [e for j, e in enumerate(expect) if j != k], (k, where)
            assert got[k] == bytes([0xA5] * 32)            # not written
    rc, st, got = var_many(L, ctx, good)                    # the context then runs a clean batch
    assert rc == SP_OK and st == [SP_OK] * K and got == expect


@pytest.mark.parametrize("n", [1, 65, 300])
def test_a_batch_of_one_is_the_single_call(L, ctx, orc, n):
    (p, s), = make_batch(orc, n, 1, 2)
    rc, st, got = var_many(L, ctx, [(p, s)])
    assert (rc, st) == (SP_OK, [SP_OK]) and (0, got[0]) == var_one(L, ctx, p, s)
    ps = Points(L, ctx, p)
    try:
        rc, got = ps.many([s])
        assert rc == SP_OK and (0, got[0]) == ps.one(s)
    finally:
        ps.free()


def test_invalid_arguments(L, ctx, orc):
    """every SP_EINVAL case of both calls. The one that cannot be reached on a box with a single GPU is a resident set that lives on ANOTHER
    device than the context: it is exercised only where the HIP runtime reports more than one device, and is NOT covered elsewhere."""
    pts = M.points(orc, 2)
    p = b"".join(pts) * 2; S = mont_array([1, 2, 3, 4]); out = (ctypes.c_uint8 * 64)(); st = (ctypes.c_int32 * 2)()
    call = lambda c=ctx.h, p=p, S=S, n=2, K=2, out=out, st=st: L.sp_msm_var_many(c, p, S, sz(n), sz(K), out, st)
    assert call() == SP_OK and list(st) == [0, 0]
    assert bytes(out) == M.oracle_msm(orc, pts, [1, 2]) + M.oracle_msm(orc, pts, [3, 4])
    assert call(c=None) == SP_EINVAL and call(p=None) == SP_EINVAL and call(S=None) == SP_EINVAL and call(out=None) == SP_EINVAL and call(st=None) == SP_EINVAL
    assert call(K=0) == SP_EINVAL and call(n=0) == SP_EINVAL
    assert call(n=MAX_N + 1, K=1) == SP_EINVAL          # rejected before anything is read
    assert call(n=1, K=MAX_K + 1) == SP_EINVAL
    assert call(n=MAX_TERMS // MAX_K + 1, K=MAX_K) == SP_EINVAL and call(n=MAX_N, K=MAX_TERMS // MAX_N + 1) == SP_EINVAL
    ps = Points(L, ctx, pts)
    try:
        pcall = lambda c=ctx.h, h=ps.h, S=S, n=2, K=2, out=out: L.sp_msm_points_many(c, h, S, sz(n), sz(K), out)
        assert pcall() == SP_OK and bytes(out) == M.oracle_msm(orc, pts, [1, 2]) + M.oracle_msm(orc, pts, [3, 4])
        assert pcall(c=None) == SP_EINVAL and pcall(h=None) == SP_EINVAL and pcall(S=None) == SP_EINVAL and pcall(out=None) == SP_EINVAL
        assert pcall(K=0) == SP_EINVAL and pcall(n=0) == SP_EINVAL and pcall(K=MAX_K + 1) == SP_EINVAL
        assert pcall(n=1) == SP_EINVAL and pcall(n=3) == SP_EINVAL            # not the set's size
    finally:
        ps.free()
    big = M.points(orc, MAX_TERMS // MAX_K + 1)         # the n K cap needs a set of more than 2^20 / 256 points
    ps = Points(L, ctx, big)
    try:
        n = len(big)
        assert L.sp_msm_points_many(ctx.h, ps.h, S, sz(n), sz(MAX_K), out) == SP_EINVAL          # n K > 2^20: rejected before anything is read
        assert L.sp_msm_points_many(ctx.h, ps.h, S, sz(n), sz(MAX_K + 1), out) == SP_EINVAL
        vecs = [rand_scalars(random.Random(k), n, KINDS[k]) for k in range(2)]                   # the same set is fine below the cap
        assert ps.many(vecs) == (SP_OK, [want(orc, big, v) for v in vecs])
    finally:
        ps.free()
    ndev = ctypes.c_int(0)                              # a set that lives on another device, where the box has one (the HIP runtime the library loaded)
    assert ctypes.CDLL("libamdhip64.so").hipGetDeviceCount(ctypes.byref(ndev)) == 0
    if ndev.value > 1:
        from spartan_amd import capi
        other = capi.Ctx(1)
        ps = Points(L, ctx, pts)
        try:
            assert L.sp_msm_points_many(other.h, ps.h, S, sz(2), sz(2), out) == SP_EINVAL
        finally:
            ps.free(); other.close()


def test_one_call_is_one_profile_record_and_one_trip(L, ctx, orc):
    n, K = 300, 3
    batch = make_batch(orc, n, K, 1)
    pts = M.points(orc, n)
    ps = Points(L, ctx, pts)
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        t0 = L.sp_ctx_trips(ctx.h)
        rc, st, _ = var_many(L, ctx, batch)
        t1 = L.sp_ctx_trips(ctx.h)
        prof = ctx.prof_read()
        assert rc == SP_OK and t1 - t0 == 1
        assert prof["msm_var"]["launches"] == 1 and prof["msm_var"]["alg_bytes"] == 64 * n * K + 32 * K and prof["msm_var"]["ms"] > 0
        assert prof["msm_points"]["launches"] == 0
        ctx.prof_reset()
        t0 = L.sp_ctx_trips(ctx.h)
        rc, _ = ps.many([s for _, s in batch])
        t1 = L.sp_ctx_trips(ctx.h)
        prof = ctx.prof_read()
        assert rc == SP_OK and t1 - t0 == 1
        assert prof["msm_points"]["launches"] == 1 and prof["msm_points"]["alg_bytes"] == 32 * n * K + 32 * K and prof["msm_points"]["ms"] > 0
        assert prof["msm_var"]["launches"] == 0
    finally:
        ctx.prof_enable(False)
        ps.free()
