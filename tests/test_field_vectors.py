"""The edge-case vectors of tests/field_vectors.py on the CPU: every generator's predicates hold and every rare-path class is populated; the
Python integer models, the product's generic (u128) arithmetic compiled for the host (hostcheck) and the oracle agree on ALL the vectors —
which pins the expected values of tests/test_gpu_field_lanes.py before a GPU is involved, and closes the same edge gap for the generic code;
and the device microkernel library (tests/csrc/devcheck.hip) cross-compiles for gfx950 in both of its builds and exports every entry point.

No pair with a Montgomery value t = (ab + mq) / 2^256 equal to q exists (field_vectors module docstring: it would need q | ab); the search
is asserted to meet none."""
import ctypes, os, re, subprocess
import pytest
from tests import field_vectors as V
from tests.helpers import *

u8x32 = ctypes.c_uint8 * 32


def _limbs(x):
    return u64x4(*[(x >> (64 * i)) & (2**64 - 1) for i in range(4)])


def _int(buf):
    return int.from_bytes(bytes(buf), "little")


def _all_vectors(family):
    """every class vector of the family plus the fillers, tagged with the class name"""
    C, _ = V.family_classes(family)
    return [(name, a, b) for name, vs in C.items() for a, b in vs] + [("filler", a, b) for a, b in V.fillers(family)]


@pytest.mark.parametrize("family", ["fq", "fp", "pt"])
def test_every_class_is_populated_and_takes_its_path(family):
    C, PRED = V.family_classes(family)
    V.check_classes(C, PRED, Q if family == "fq" else None)       # the predicate of every class on every vector (also asserted by the generators)
    assert set(C) == set(PRED)
    n = {k: len(v) for k, v in C.items()}
    if family == "fq":
        assert n["t_in_[q,2q)"] >= 256 and n["special_pairs"] == 16 * 16
        assert all(n["m%d_%s" % (i, t)] >= 1 for i in range(8) for t in ("zero", "ones"))
        assert all(n["sum_ffff_carry_w%d" % k] >= 1 for k in range(7)) and all(n["diff_zero_borrow_w%d" % k] >= 1 for k in range(1, 8))
        for a, b in C["t_in_[q,2q)"]:
            assert V.mont_t(a, b) != Q
        assert sum(1 for a, b in C["special_pairs"] if V.mont_t(a, b) >= Q) >= 1
    elif family == "fp":
        assert n["mul_second_fold"] >= 256 and n["sqr_second_fold"] >= 256 and n["mul_special_pairs"] == 12 * 12
        assert all(n["sum_ffff_carry_w%d" % k] >= 1 for k in range(8))
        assert max(V.fp_fold(a, b)[0] for a, b in C["mul_fold1_cmax38"]) == 38
        assert V.fp_add_raw_model(2**256 - 1, 2**256 - 1) == 74 and V.fp_sub_raw_model(0, 2**256 - 1) == 2**256 - 75
    else:
        assert n["bad_a"] == 29 and n["bad_b"] == 29 and n["rfc_multiples"] == 16


def test_uniform_pairs_almost_never_take_the_rare_paths():
    """why the classes exist: of 20000 uniform pairs none takes fp_mul's second fold, and about one in 70 a Montgomery value in [q, 2q)"""
    import random
    rng = random.Random(5)
    assert sum(V.fp_fold(rng.getrandbits(256), rng.getrandbits(256))[1] for _ in range(20000)) == 0
    hits = sum(V.mont_t(rng.randrange(Q), rng.randrange(Q)) >= Q for _ in range(20000))
    assert 100 < hits < 600


def test_layouts_cover_every_class():
    for family in ("fq", "fp", "pt"):
        C, _ = V.family_classes(family)
        a, b, c = V.layout_a(family), V.layout_b(family), V.layout_c(family)
        assert {x[0] for x in a} == set(C) | {"filler"}
        assert len(b) == 64 * len(V.LANES_B) * len(C) and len(c) % 64 == 0
        for w in range(len(b) // 64):   # one edge vector per wavefront, at the lane it is meant for
            wave = b[64 * w:64 * w + 64]
            edge = [i for i, x in enumerate(wave) if x[0] != "filler"]
            assert edge == [V.LANES_B[w % len(V.LANES_B)]]
        for w in range(len(c) // 64):
            assert len(set(c[64 * w:64 * w + 64])) == 1
        for n in V.SIZES_D:             # (d): every class at every size, and an edge vector in the lone lane of a partial wavefront
            runs = V.layout_d(family, n)
            assert all(len(r) == n for r in runs)
            assert {x[0] for r in runs for x in r} - {"filler"} == set(C), (family, n)
            assert all(r[0][0] != "filler" and r[(n - 1) // 64 * 64][0] != "filler" for r in runs)
            assert runs == V.layout_d(family, n)
        assert max(len(a), len(b), len(c)) < 2**18
        assert a == V.layout_a(family)   # seeded: the same vectors every run


def test_python_point_model_gives_the_rfc_multiples():
    from tests.test_oracle_pins import RFC_MULTIPLES
    m = V.pt_material()
    assert [V.pt_encode(p).to_bytes(32, "little").hex() for p in m["mult"]] == RFC_MULTIPLES
    assert V.INVSQRT_A_MINUS_D == 54469307008909316920995813868745141605393597292927456921205312896311721017578   # RFC 9496 4.1
    assert all(V.pt_encode(V.pt_decode(V.pt_encode(p))) == V.pt_encode(p) for p in m["generic"][:8])   # up to the ristretto coset


@pytest.mark.parametrize("op", sorted(V.OPS))
def test_host_generic_code_matches_python_on_all_vectors(hc, op):
    """hc_<op>_n: the wrappers of tests/csrc/checkops.hpp (what the device microkernels run) over the generic host forms"""
    vec = _all_vectors(V.OPS[op][0])
    n = len(vec)
    out = ctypes.create_string_buffer(32 * n)
    getattr(hc, "hc_%s_n" % op)(V.pack([a for _, a, _ in vec]), V.pack([b for _, _, b in vec]), out, sz(n))
    bad = []
    for i, (name, a, b) in enumerate(vec):
        got, want = int.from_bytes(out.raw[32 * i:32 * i + 32], "little"), V.expect(op, a, b)
        if got != want:
            bad.append("%s[%s] a=%#x b=%#x want %#x got %#x" % (op, name, a, b, want, got))
        if op.startswith("fq_"):
            assert got < Q, (op, name)
    assert not bad, "%d of %d differ:\n%s" % (len(bad), n, "\n".join(bad[:10]))


def test_single_element_shims_and_oracle_agree_on_all_fq_vectors(hc, orc):
    o1, o2 = u64x4(), u64x4()
    vec = _all_vectors("fq")
    for name, a, b in vec:
        la, lb = _limbs(a), _limbs(b)
        for op in ("add", "sub", "mul"):
            getattr(hc, "hc_fq_" + op)(la, lb, o1); getattr(orc, "orc_fq_" + op)(la, lb, o2)
            assert _int(o1) == _int(o2) == V.expect("fq_" + op, a, b), (op, name, hex(a), hex(b))
        hc.hc_fq_neg(la, o1); orc.orc_fq_neg(la, o2); assert _int(o1) == _int(o2) == V.expect("fq_neg", a, b), (name, hex(a))
        hc.hc_fq_dbl(la, o1); assert _int(o1) == V.expect("fq_dbl", a, b), (name, hex(a))
        hc.hc_fq_sqr(la, o1); assert _int(o1) == V.expect("fq_sqr", a, b), (name, hex(a))
        hc.hc_fq_from_mont(la, o1); assert _int(o1) == V.expect("fq_from_mont", a, b), (name, hex(a))
        hc.hc_fq_to_mont(la, o1); assert _int(o1) == V.expect("fq_to_mont", a, b), (name, hex(a))
        hc.hc_fq_invert(la, o1); orc.orc_fq_invert(la, o2); assert _int(o1) == _int(o2) == V.expect("fq_invert", a, b), (name, hex(a))


def test_single_element_shims_agree_on_all_fp_vectors(hc):
    out = u8x32()
    for name, a, b in _all_vectors("fp"):
        la, lb = _limbs(a), _limbs(b)
        hc.hc_fp_add_raw(la, lb, out); assert _int(out) == (a + b) % P, (name, hex(a), hex(b))
        hc.hc_fp_sub_raw(la, lb, out); assert _int(out) == (a - b) % P, (name, hex(a), hex(b))
        hc.hc_fp_mul_raw(la, lb, out); assert _int(out) == a * b % P, (name, hex(a), hex(b))
        hc.hc_fp_sqr_raw(la, out); assert _int(out) == a * a % P, (name, hex(a))
        hc.hc_fp_neg_raw(la, out); assert _int(out) == (-a) % P, (name, hex(a))
        assert V.fp_add_raw_model(a, b) % P == (a + b) % P and V.fp_sub_raw_model(a, b) % P == (a - b) % P
        assert 0 <= V.fp_add_raw_model(a, b) < 2**256 and 0 <= V.fp_sub_raw_model(a, b) < 2**256


def test_points_python_hostcheck_and_oracle_agree(hc, orc):
    o1, o2 = u8x32(), u8x32()
    for name, a, b in _all_vectors("pt"):
        ba, bb = a.to_bytes(32, "little"), b.to_bytes(32, "little")
        for fn, op, args in (("pt_recompress", "pt_recompress", (ba,)), ("pt_add", "pt_add", (ba, bb)), ("pt_dbl", "pt_dbl", (ba,))):
            want = V.expect(op, a, b)
            r1 = getattr(hc, "hc_" + fn)(*args, o1); r2 = getattr(orc, "orc_" + fn)(*args, o2)
            assert (r1, r2) == ((0, 0) if want == V.BAD else (1, 1)), (fn, name, hex(a), hex(b))
            if want != V.BAD:
                assert _int(o1) == _int(o2) == want, (fn, name, hex(a), hex(b))
        for neg in (0, 1):
            want = V.expect("pt_madd%d" % neg, a, b)
            r = hc.hc_pt_madd(ba, bb, ctypes.c_int(neg), o1)
            assert r == (0 if want == V.BAD else 1) and (want == V.BAD or _int(o1) == want), (neg, name, hex(a), hex(b))


def test_devcheck_has_no_assembly_of_its_own():
    for f in ("devcheck.hip", "checkops.hpp"):
        src = open(os.path.join(ROOT, "tests", "csrc", f)).read()
        assert not re.search(r"\basm\b|__asm|\basm\s*\(", src), f
        assert "asm" not in src, f


@pytest.mark.parametrize("generic", [False, True])
def test_devcheck_cross_compiles_and_exports_every_entry_point(generic):
    L = load_devcheck(generic)      # builds for gfx950 when missing or stale; loading needs no GPU
    for op in V.OPS:
        assert hasattr(L, "dc_" + op), op
    assert L.dc_flags() == (7 if generic else 0)
    so = os.path.join(ROOT, "tests", "csrc", "libdevcheck%s.so" % ("_generic" if generic else ""))
    assert b"gfx950" in open(so, "rb").read()
    # the list of operations is the one of checkops.hpp, entry for entry, with the same divergent-mode partner
    src = open(os.path.join(ROOT, "tests", "csrc", "checkops.hpp")).read()
    listed = re.findall(r"X\((\w+), (\w+)_op, (\w+)_op\)", src)
    assert {(n, alt) for n, _, alt in listed} == {(n, v[1]) for n, v in V.OPS.items()} and all(n == o for n, o, _ in listed)
