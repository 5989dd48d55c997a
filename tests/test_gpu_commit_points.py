"""sp_commit_rows_points (spartan_amd/csrc/msm_var.hip): the row commitments of a device table over a range of a resident point set, byte for
byte against the oracle's orc_commit_rows on the set's own encodings (h = the identity, no blinds), against sp_msm_points_range row by row
and, where a shape is too large for the oracle, against sp_commit_rows_dev over an sp_gens made from the same uniform bytes. The launch plan
has one threshold, the slice of 256 columns a block sums: cols 255 | 256 | 257, 511 | 512 | 513 and 1024 sit on it; rows are flattened with
the slices on gridDim.x (65535 | 65536 rows). Scalars end the digit walk early (small), never (uniform, q - 1) and carry through every window."""
import ctypes, hashlib, random
import pytest
from tests.helpers import *
from tests import msm_var_cases as M

pytestmark = pytest.mark.gpu
SP_EINVAL = -1
KINDS = ["uniform", "sparse", "small", "edge"]
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")
COUNT = 1026
NIB8, NIB9 = int("8" * 64, 16), int("9" * 64, 16)
# every digit 8 without a carry / every nibble 9: digit -7 and a carry into the next window, through all 64 (the forms below q: 63 nibbles)
CARRY = [1, 8, 9, 2**252, Q - 1, NIB8 % Q, NIB9 % Q, int("8" * 63, 16) % 2**252, int("9" * 63, 16) % 2**252]
# (cols, rows, off, z_off): off "end" = count - cols. Every value of each axis occurs; both sides of the 256-column slice occur with 1 and with
# several rows, at off 0 and at an odd off
SHAPES = [(1, 17, 0, 0), (2, 3, 1, 5), (63, 2, "end", 0), (64, 1, 0, 5), (65, 17, 1, 0), (255, 3, "end", 5), (256, 2, 0, 0), (257, 17, 1, 5),
          (511, 1, "end", 0), (512, 3, 0, 5), (513, 2, 1, 0), (1024, 17, "end", 5), (1024, 1, 0, 0), (256, 17, "end", 5), (257, 1, 0, 0),
          (1, 1, "end", 5), (255, 1, 1, 0), (256, 1, 1, 5), (513, 3, "end", 5)]
assert all(r * c <= 20000 for c, r, _, _ in SHAPES)


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


def uniform_bytes(n):
    return hashlib.shake_256(b"gens_r1cs_eval" + BASEPOINT).digest(64 * n)


class Set:
    """a resident point set from the generator stream's uniform bytes, or from encodings"""
    def __init__(self, L, ctx, n=None, pts=None):
        self.L, self.ctx, self.h = L, ctx, vp()
        if pts is None:
            out = (ctypes.c_uint8 * (32 * n))()
            assert L.sp_points_from_uniform(ctx.h, uniform_bytes(n), sz(n), out, ctypes.byref(self.h)) == 0
            self.n, self.comp = n, bytes(out)
        else:
            assert L.sp_points_upload(ctx.h, b"".join(pts), sz(len(pts)), ctypes.byref(self.h)) == 0
            self.n, self.comp = len(pts), b"".join(pts)

    def commit(self, off, tab, z_off, rows, cols):
        out = (ctypes.c_uint8 * (32 * rows))(*([0xA5] * (32 * rows)))
        rc = self.L.sp_commit_rows_points(self.ctx.h, self.h, sz(off), tab.h if tab is not None else None, sz(z_off), sz(rows), sz(cols), out)
        return rc, bytes(out)

    def row(self, off, scalars):
        out = (ctypes.c_uint8 * 32)()
        assert self.L.sp_msm_points_range(self.ctx.h, self.h, sz(off), sz(len(scalars)), mont_bulk(scalars), out) == 0
        return bytes(out)

    def free(self):
        if self.h:
            self.L.sp_points_free(self.h); self.h = vp()


@pytest.fixture(scope="module")
def big(L, ctx):
    s = Set(L, ctx, COUNT)
    yield s
    s.free()


def table(ctx, Z, z_off, tail=7):
    """Z at [z_off, z_off + len(Z)) of a longer table whose other entries are q - 1: a read past either end changes the bytes"""
    from spartan_amd import capi
    full = [Q - 1] * z_off + list(Z) + [Q - 1] * tail
    return capi.Table.upload(ctx, mont_bulk(full), len(full))


def oracle_rows(orc, comp, off, Z, rows, cols):
    want = (ctypes.c_uint8 * (32 * rows))()
    assert orc.orc_commit_rows(comp[32 * off:32 * (off + cols)], sz(cols), M.IDENTITY, mont_bulk(Z), sz(rows), sz(cols), None, want) == 0
    return bytes(want)


def check(orc, s, Z, rows, cols, off, z_off, per_row=True):
    tab = table(s.ctx, Z, z_off)
    try:
        rc, got = s.commit(off, tab, z_off, rows, cols)
    finally:
        tab.free()
    assert rc == 0, (rows, cols, off, z_off, rc)
    want = oracle_rows(orc, s.comp, off, Z, rows, cols)
    bad = [r for r in range(rows) if got[32 * r:32 * r + 32] != want[32 * r:32 * r + 32]]
    assert not bad, (rows, cols, off, z_off, bad)
    if per_row:
        for r in range(rows):
            assert got[32 * r:32 * r + 32] == s.row(off, Z[r * cols:(r + 1) * cols]), (rows, cols, off, z_off, r)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_r%d_%s_z%d" % s)
def test_shapes_match_the_oracle_and_the_row_calls(big, orc, shape):
    cols, rows, off, z_off = shape
    off = COUNT - cols if off == "end" else off
    k0 = SHAPES.index(shape)
    rng = random.Random(1000 * cols + rows)
    Z = [x for r in range(rows) for x in rand_scalars(rng, cols, KINDS[(r + k0) % 4])]
    check(orc, big, Z, rows, cols, off, z_off)


def test_axes_are_covered():
    assert {c for c, _, _, _ in SHAPES} == {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024}
    assert {r for _, r, _, _ in SHAPES} == {1, 2, 3, 17} and {o for _, _, o, _ in SHAPES} == {0, 1, "end"} and {z for _, _, _, z in SHAPES} == {0, 5}
    for side in (255, 256, 257):          # the slice threshold with one row and with several
        assert {r > 1 for c, r, _, _ in SHAPES if c == side} == {False, True}


@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_of_scalar_fills_a_matrix(big, orc, kind):
    rows, cols = 3, 257
    Z = rand_scalars(random.Random(KINDS.index(kind)), rows * cols, kind)
    check(orc, big, Z, rows, cols, 2, 5)


def test_special_rows(big, orc):
    """an all-zero row, a row whose only entry is its last column, rows alternately short and full (SPARK's comb_ops), and the carry cases"""
    cols, rng = 300, random.Random(42)
    rows_ = [[0] * cols, [0] * (cols - 1) + [rng.randrange(1, Q)]]
    for r in range(4):
        rows_.append(rand_scalars(rng, cols, "small" if r % 2 == 0 else "uniform"))
    rows_ += [[v] * cols for v in CARRY]
    rows_.append([CARRY[i % len(CARRY)] for i in range(cols)])
    Z = [x for row in rows_ for x in row]
    assert len(Z) <= 20000
    got = check(orc, big, Z, len(rows_), cols, 1, 5)
    assert got[:32] == M.IDENTITY
    last = big.row(1 + cols - 1, [rows_[1][-1]])
    assert got[32:64] == last != M.IDENTITY


@pytest.mark.parametrize("n", [64, 257])
def test_untrusted_points(L, ctx, orc, n):
    """repeats, adjacent and distant negatives, the identity among the inputs: one-row commitments over uploaded sets"""
    rng = random.Random(n)
    for name, pts, S in M.named_cases(orc, rng, n):
        s = Set(L, ctx, pts=list(pts))
        tab = table(ctx, S, 5)
        try:
            rc, got = s.commit(0, tab, 5, 1, n)
            assert rc == 0, (name, rc)
            assert got == M.oracle_msm(orc, pts, S), (name, n)
            assert got == s.row(0, S), (name, n)
            if name in ("all_zero", "only_a_pair_of_negatives"):
                assert got == M.IDENTITY, name
        finally:
            tab.free(); s.free()


class DeviceReference:
    """sp_commit_rows_dev over the fixed-base tables of the same stream's first n points (8-bit windows: small tables)"""
    def __init__(self, ctx, n):
        from spartan_amd import capi
        ctx.set_option("msm.wbits", 8)
        try:
            self.g = capi.Gens(ctx, uniform=uniform_bytes(n))
        finally:
            ctx.set_option("msm.wbits", 0)

    def rows(self, L, ctx, tab, off, rows, cols):
        out = (ctypes.c_uint8 * (32 * rows))()
        assert L.sp_commit_rows_dev(ctx.h, self.g.h, sz(off), sz(0), tab.h, sz(0), sz(rows), sz(cols), None, out) == 0
        return bytes(out)


@pytest.mark.parametrize("rows", [65535, 65536])
def test_rows_at_the_bound_against_the_device_reference(L, ctx, big, rows):
    """rows beyond the 65535 of a grid's y and z: they are flattened on x"""
    from spartan_amd import capi
    ref = DeviceReference(ctx, 2)
    Z = rand_scalars(random.Random(rows), rows, "small")
    tab = capi.Table.upload(ctx, mont_bulk(Z), rows)
    try:
        assert ref.g.compressed == big.comp[:64]
        rc, got = big.commit(1, tab, 0, rows, 1)
        assert rc == 0
        assert got == ref.rows(L, ctx, tab, 1, rows, 1)
        for r in (0, rows // 2, rows - 1):      # and the second point really is the base
            assert got[32 * r:32 * r + 32] == big.row(1, [Z[r]])
    finally:
        tab.free(); ref.g.free()


def test_a_row_of_the_2p20_commitment_against_the_device_reference(L, ctx):
    """cols = 4096 (16 slices) at off 0 and off 2 of a 4098-point set: a full row and a short row"""
    from spartan_amd import capi
    n, cols = 4098, 4096
    s = Set(L, ctx, n)
    ref = DeviceReference(ctx, n)
    rng = random.Random(4096)
    Z = fast_scalars(rng, cols) + rand_scalars(rng, cols, "small")
    tab = capi.Table.upload(ctx, mont_bulk(Z), 2 * cols)
    try:
        assert ref.g.compressed == s.comp
        for off in (0, 2):
            rc, got = s.commit(off, tab, 0, 2, cols)
            assert rc == 0, off
            assert got == ref.rows(L, ctx, tab, off, 2, cols), off
            assert got[32:] == s.row(off, Z[cols:]), off
    finally:
        tab.free(); ref.g.free(); s.free()


def test_refusals_leave_out_untouched(L, ctx, big, orc):
    """every SP_EINVAL of the contract that one device can show (a set or a table on another device than the context needs two)"""
    from spartan_amd import capi
    rows, cols, z_off = 3, 300, 5
    Z = rand_scalars(random.Random(7), rows * cols)
    tab = table(ctx, Z, z_off)                       # z_off + rows * cols + 7 entries
    long_tab = capi.Table.alloc(ctx, 65537)
    n_tab = z_off + rows * cols + 7
    untouched = bytes([0xA5]) * (32 * rows)
    try:
        assert L.sp_table_len(tab.h) == n_tab
        refused = [
            big.commit(0, tab, z_off, 0, cols), big.commit(0, tab, z_off, rows, 0),                       # rows = 0, cols = 0
            big.commit(COUNT - cols + 1, tab, z_off, rows, cols), big.commit(COUNT, tab, z_off, 1, 1),    # off + cols = count + 1
            big.commit(2**64 - 1, tab, z_off, rows, 2), big.commit(0, tab, z_off, 1, COUNT + 1),          # ... wrapping; more columns than points
            big.commit(0, tab, z_off + 8, rows, cols), big.commit(0, tab, n_tab, 1, 1),                   # z_off + rows cols = len + 1
            big.commit(0, tab, 2**64 - 1, rows, cols), big.commit(0, tab, 2**64 - rows * cols + 1, rows, cols),   # ... wrapping
            big.commit(0, tab, n_tab + 1, 1, 1),
            big.commit(0, None, z_off, rows, cols),
        ]
        for rc, out in refused:
            assert rc == SP_EINVAL and out == untouched[:len(out)]
        out = (ctypes.c_uint8 * (32 * rows))(*([0xA5] * (32 * rows)))
        assert L.sp_commit_rows_points(None, big.h, sz(0), tab.h, sz(z_off), sz(rows), sz(cols), out) == SP_EINVAL
        assert L.sp_commit_rows_points(ctx.h, None, sz(0), tab.h, sz(z_off), sz(rows), sz(cols), out) == SP_EINVAL
        assert L.sp_commit_rows_points(ctx.h, big.h, sz(0), tab.h, sz(z_off), sz(rows), sz(cols), None) == SP_EINVAL
        assert bytes(out) == untouched
        big_out = (ctypes.c_uint8 * (32 * 65537))(*([0xA5] * (32 * 65537)))
        assert L.sp_commit_rows_points(ctx.h, big.h, sz(0), long_tab.h, sz(0), sz(65537), sz(1), big_out) == SP_EINVAL     # rows > 65536
        assert bytes(big_out) == bytes([0xA5]) * (32 * 65537)
        # and a valid call gives the right bytes afterwards, with the table's last entry the call's last
        check(orc, big, Z, rows, cols, 0, z_off, per_row=False)
        rc, got = big.commit(COUNT - 1, tab, n_tab - 1, 1, 1)
        assert rc == 0 and got == big.row(COUNT - 1, [Q - 1])
    finally:
        tab.free(); long_tab.free()
