"""sp_points / sp_msm_points (spartan_amd/csrc/msm_var.hip): the multi-scalar multiplication over a resident point set, byte for byte against the
oracle's orc_pt_msm and against sp_msm_var on the same inputs. Sizes sit on the kernels' edges: a wavefront (64), a block of the window-sum
kernel (256), finishing blocks of 64, 256 (its 256 lanes exactly full), 320 (the first uneven stride), 1024 and 1088 partial sums, and the two
sizes next to where the call's 32 n bytes of scalars leave the host-mapped page for the staging buffer (HMAP_GEN, read from internal.hpp)."""
import ctypes, random
import pytest
from tests.helpers import *
from tests import msm_var_cases as M
from tests.test_gpu_msm_many import hmap_gen

pytestmark = pytest.mark.gpu
PAGE_N = hmap_gen() // 32      # the last n whose scalars are read from the host-mapped page; PAGE_N + 1 is staged on the device
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 4096, 4097,
         pytest.param(PAGE_N, id="last_size_on_the_host_page"), pytest.param(PAGE_N + 1, id="first_size_off_the_host_page")]
KINDS = ["uniform", "sparse", "small", "edge"]
SP_EINVAL, SP_EPOINT = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    c = capi.Ctx(0)
    yield c
    c.close()


class Points:
    def __init__(self, ctx, pts):
        from spartan_amd import capi
        self.L, self.ctx, self.n, self.h = capi.lib, ctx, len(pts), vp()
        self.rc = self.L.sp_points_upload(ctx.h, b"".join(pts), sz(len(pts)), ctypes.byref(self.h))

    def msm(self, scalars):
        out = (ctypes.c_uint8 * 32)()
        rc = self.L.sp_msm_points(self.ctx.h, self.h, mont_array(scalars), sz(len(scalars)), out)
        return rc, bytes(out)

    def free(self):
        if self.h:
            self.L.sp_points_free(self.h); self.h = vp()


def msm_var(ctx, pts, scalars):
    from spartan_amd import capi
    out = (ctypes.c_uint8 * 32)()
    rc = capi.lib.sp_msm_var(ctx.h, b"".join(pts), mont_array(scalars), sz(len(pts)), out)
    return rc, bytes(out)


@pytest.mark.parametrize("n", SIZES)
def test_matches_oracle_and_msm_var_at_every_reduction_edge(ctx, orc, n):
    """one set per size, all four kinds of scalars over it ("edge" reaches the carry into the 64th signed digit)"""
    pts = M.points(orc, n)
    ps = Points(ctx, pts)
    assert ps.rc == 0 and ps.L.sp_points_count(ps.h) == n
    try:
        for kind in KINDS:
            rng = random.Random(1000 * n + KINDS.index(kind))
            S = rand_scalars(rng, n, kind)
            rc, got = ps.msm(S)
            assert rc == 0, (n, kind, rc)
            assert got == M.oracle_msm(orc, pts, S), (kind, n)
            assert (0, got) == msm_var(ctx, pts, S), (kind, n)
    finally:
        ps.free()


@pytest.mark.parametrize("n", [64, 257])
def test_named_cases(ctx, orc, n):
    """the identity, repeats and mutual negatives are legal members of a set (all-zero rows of comb_mem commit to the identity)"""
    rng = random.Random(n)
    for name, pts, S in M.named_cases(orc, rng, n):
        ps = Points(ctx, pts)
        try:
            assert ps.rc == 0, (name, ps.rc)
            rc, got = ps.msm(S)
            assert rc == 0, (name, rc)
            assert got == M.oracle_msm(orc, pts, S), (name, n)
            assert (0, got) == msm_var(ctx, pts, S), (name, n)
            if name in ("all_zero", "only_a_pair_of_negatives"):
                assert got == M.IDENTITY, name
        finally:
            ps.free()


def test_a_set_is_reused_and_calls_leave_nothing_behind(ctx, orc):
    """one set under three scalar vectors, another set's multiplication in between: the results are those of the first round"""
    rng = random.Random(9)
    pts, other = M.points(orc, 300), M.points(orc, 1025, seed=3)
    a, b = Points(ctx, pts), Points(ctx, other)
    try:
        assert a.rc == 0 and b.rc == 0
        vecs = [rand_scalars(rng, 300, k) for k in ("uniform", "edge", "sparse")]
        So = rand_scalars(rng, 1025)
        first = [a.msm(S) for S in vecs]
        assert b.msm(So) == (0, M.oracle_msm(orc, other, So))
        for S, f in zip(vecs, first):
            assert f == (0, M.oracle_msm(orc, pts, S))
            assert a.msm(S) == f
            b.msm(So)
    finally:
        a.free(); b.free()


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_invalid_encoding_is_found_at_upload_and_the_context_survives(ctx, orc, n):
    from tests.test_oracle_pins import RFC_BAD
    rng = random.Random(n)
    good = M.points(orc, n)
    for k, where in enumerate(sorted({0, n // 2, n - 1})):
        pts = list(good)
        pts[where] = bytes.fromhex(RFC_BAD[(k * 7 + n) % len(RFC_BAD)])
        ps = Points(ctx, pts)
        assert ps.rc == SP_EPOINT and not ps.h, (n, where, ps.rc)
    if n == 1:
        for enc in RFC_BAD:     # every class of RFC 9496 A.2
            assert Points(ctx, [bytes.fromhex(enc)]).rc == SP_EPOINT, enc
    ps = Points(ctx, good)
    S = rand_scalars(rng, n)
    try:
        assert ps.rc == 0 and ps.msm(S) == (0, M.oracle_msm(orc, good, S))
    finally:
        ps.free()


def test_invalid_arguments(ctx, orc):
    from spartan_amd import capi
    L = capi.lib
    out = (ctypes.c_uint8 * 32)()
    pts = M.points(orc, 2)
    p = b"".join(pts); S = mont_array([1, 2]); h = vp()
    assert L.sp_points_upload(None, p, sz(2), ctypes.byref(h)) == SP_EINVAL
    assert L.sp_points_upload(ctx.h, None, sz(2), ctypes.byref(h)) == SP_EINVAL
    assert L.sp_points_upload(ctx.h, p, sz(2), None) == SP_EINVAL
    assert L.sp_points_upload(ctx.h, p, sz(0), ctypes.byref(h)) == SP_EINVAL
    assert L.sp_points_upload(ctx.h, p, sz(65537), ctypes.byref(h)) == SP_EINVAL and not h
    assert L.sp_points_count(None) == 0
    L.sp_points_free(None)
    ps = Points(ctx, pts)
    try:
        assert ps.rc == 0
        assert L.sp_msm_points(None, ps.h, S, sz(2), out) == SP_EINVAL
        assert L.sp_msm_points(ctx.h, None, S, sz(2), out) == SP_EINVAL
        assert L.sp_msm_points(ctx.h, ps.h, None, sz(2), out) == SP_EINVAL
        assert L.sp_msm_points(ctx.h, ps.h, S, sz(2), None) == SP_EINVAL
        assert L.sp_msm_points(ctx.h, ps.h, S, sz(0), out) == SP_EINVAL
        assert L.sp_msm_points(ctx.h, ps.h, mont_array([1, 2, 3]), sz(3), out) == SP_EINVAL     # a scalar count that is not the set's size
        assert L.sp_msm_points(ctx.h, ps.h, S, sz(1), out) == SP_EINVAL
        assert L.sp_msm_points(ctx.h, ps.h, S, sz(2), out) == 0 and bytes(out) == M.oracle_msm(orc, pts, [1, 2])
    finally:
        ps.free()


def test_profile_family(ctx, orc):
    """one call = one recorded launch chain of the family msm_points; the upload records none, and msm_var's count stays its own"""
    rng = random.Random(5)
    pts = M.points(orc, 300)
    ctx.prof_enable(True); ctx.prof_reset()
    ps = Points(ctx, pts)
    try:
        assert ps.rc == 0
        assert ctx.prof_read()["msm_points"]["launches"] == 0
        ps.msm(rand_scalars(rng, 300))
        prof = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
        ps.free()
    fam = prof["msm_points"]
    assert fam["launches"] == 1 and fam["alg_bytes"] == 32 * 300 + 32 and fam["ms"] > 0
    assert prof["msm_var"]["launches"] == 0
