"""sp_msm_var (spartan_amd/csrc/msm_var.hip): the variable-base multi-scalar multiplication of the verifier, byte for byte against the
oracle's orc_pt_msm. Sizes sit on the kernel's edges: a wavefront (64), a block of the window-sum kernel (256), the cross-block stage
(> 256: 2, 4, 5 and 16 blocks; the finishing kernel gives 4 lanes to a window, so 5 blocks is its first uneven split), and the two sizes
next to where the call's 64 n bytes of input leave the host-mapped page for the staging buffer (HMAP_GEN, read from internal.hpp)."""
import ctypes, random
import pytest
from tests.helpers import *
from tests import msm_var_cases as M
from tests.test_gpu_msm_many import hmap_gen

pytestmark = pytest.mark.gpu
PAGE_N = hmap_gen() // 64      # the last n whose encodings and scalars are read from the host-mapped page; PAGE_N + 1 is staged on the device
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, PAGE_N, PAGE_N + 1, 1024, 1025, 4096]
SP_EINVAL, SP_EPOINT = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    c = capi.Ctx(0)
    yield c
    c.close()


def msm_var(ctx, pts, scalars, fill=0):
    from spartan_amd import capi
    out = (ctypes.c_uint8 * 32)(*([fill] * 32))
    rc = capi.lib.sp_msm_var(ctx.h, b"".join(pts), mont_array(scalars), sz(len(pts)), out)
    return rc, bytes(out)


@pytest.mark.parametrize("kind", ["uniform", "sparse", "small", "edge"])
def test_matches_oracle_at_every_reduction_edge(ctx, orc, kind):
    rng = random.Random({"uniform": 1, "sparse": 2, "small": 3, "edge": 4}[kind])
    for n in SIZES:
        pts = M.points(orc, n)
        S = rand_scalars(rng, n, kind)
        rc, got = msm_var(ctx, pts, S)
        assert rc == 0, (n, rc)
        assert got == M.oracle_msm(orc, pts, S), (kind, n)


@pytest.mark.parametrize("n", [64, 257])
def test_named_cases(ctx, orc, n):
    rng = random.Random(n)
    for name, pts, S in M.named_cases(orc, rng, n):
        rc, got = msm_var(ctx, pts, S)
        assert rc == 0, (name, rc)
        assert got == M.oracle_msm(orc, pts, S), (name, n)
        if name in ("all_zero", "only_a_pair_of_negatives"):
            assert got == M.IDENTITY, name


def test_result_does_not_depend_on_what_ran_before(ctx, orc):
    """the same call twice, with another size in between: the scratch of one call leaves nothing behind for the next"""
    rng = random.Random(9)
    pts = M.points(orc, 300); S = rand_scalars(rng, 300)
    _, a = msm_var(ctx, pts, S)
    msm_var(ctx, M.points(orc, 1025), rand_scalars(rng, 1025))
    _, b = msm_var(ctx, pts, S)
    assert a == b == M.oracle_msm(orc, pts, S)


@pytest.mark.parametrize("n", [1, 65, 1025, pytest.param(PAGE_N + 1, id="first_size_off_the_host_page")])
def test_invalid_encoding_is_reported_and_the_context_survives(ctx, orc, n):
    """SP_EPOINT wherever the bad point sits (the last index included), `out` as the caller left it, and the next call is correct"""
    from tests.test_oracle_pins import RFC_BAD
    rng = random.Random(n)
    good = M.points(orc, n)
    S = rand_scalars(rng, n)
    for k, where in enumerate(sorted({0, n // 2, n - 1})):
        pts = list(good)
        pts[where] = bytes.fromhex(RFC_BAD[(k * 7 + n) % len(RFC_BAD)])
        rc, out = msm_var(ctx, pts, S, fill=0xA5)
        assert rc == SP_EPOINT, (n, where, rc)
        assert out == b"\xa5" * 32, (n, where)
    if n == 1:
        for enc in RFC_BAD:     # every class of RFC 9496 A.2
            assert msm_var(ctx, [bytes.fromhex(enc)], S)[0] == SP_EPOINT, enc
    rc, got = msm_var(ctx, good, S)
    assert rc == 0 and got == M.oracle_msm(orc, good, S)


def test_invalid_arguments(ctx, orc):
    from spartan_amd import capi
    out = (ctypes.c_uint8 * 32)()
    p = b"".join(M.points(orc, 2)); S = mont_array([1, 2])
    L = capi.lib.sp_msm_var
    assert L(ctx.h, p, S, sz(0), out) == SP_EINVAL
    assert L(ctx.h, p, S, sz(65537), out) == SP_EINVAL
    assert L(None, p, S, sz(2), out) == SP_EINVAL
    assert L(ctx.h, None, S, sz(2), out) == SP_EINVAL
    assert L(ctx.h, p, None, sz(2), out) == SP_EINVAL
    assert L(ctx.h, p, S, sz(2), None) == SP_EINVAL
    assert L(ctx.h, p, S, sz(2), out) == 0 and bytes(out) == M.oracle_msm(orc, M.points(orc, 2), [1, 2])


def test_profile_family(ctx, orc):
    """one call = one recorded launch chain of the family msm_var, with its algorithmic bytes"""
    rng = random.Random(5)
    ctx.prof_enable(True); ctx.prof_reset()
    msm_var(ctx, M.points(orc, 300), rand_scalars(rng, 300))
    fam = ctx.prof_read()["msm_var"]
    ctx.prof_enable(False)
    assert fam["launches"] == 1 and fam["alg_bytes"] == 64 * 300 + 32 and fam["ms"] > 0
