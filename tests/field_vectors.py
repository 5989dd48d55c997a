"""Seeded edge-case vectors and Python-integer models for the element-wise field / curve checks (tests/csrc/checkops.hpp run on the host
by hostcheck.cc and on the device by devcheck.hip). Test infrastructure only.

Every operand and every result is one 32-byte little-endian value, held here as a Python int below 2^256:
  Fq      raw Montgomery limbs (x * 2^256 mod q), always < q — fed as they are, never through to_mont_limbs, so the 32-bit word
          patterns that steer the carry chains are under control
  Fp      raw limbs anywhere in [0, 2^256); results are canonical ([0, p)) except for the *_raw operations
  points  compressed ristretto255 encodings; a rejected encoding gives BAD (32 bytes of 0xff)

A vector CLASS is a named list of (a, b) pairs with a predicate over Python integers that says which rare path the pair takes; the
generators assert the predicate on every pair they emit (check_classes), so a class cannot silently miss its path.

Unreachable corners (proved, not searched):
  * fq_add with a sum word of 0xffffffff plus a carry-in at word 7: operands below q have top words <= 0x10000000, their sum <= 0x20000001.
    The same chain code (sp_chain2) takes that pattern at word 7 in the Fp classes, where operands are arbitrary.
  * an Fq operand with 0xffffffff in word 7 (same bound): words 0..6 only.
  * a Montgomery product with t = (ab + mq) / 2^256 equal to q exactly: it needs ab + mq = q 2^256, so q | ab, so a or b is 0 (q is prime,
    a, b < q), and then m = 0 and t = 0. fq_mul_classes asserts the search meets none.
  * fp_mul first-fold carry c > 38: N = lo + 38 hi < 39 * 2^256. c = 38 is reached (a = b = 2^256 - 1 - 2^20, say) and is a class.
"""
import random
from tests.helpers import Q, P, R, RINV

M32 = 0xffffffff
M64 = (1 << 64) - 1
W256 = 1 << 256
BAD = W256 - 1
R2 = R * R % Q
QINV256 = (-pow(Q, -1, W256)) % W256
Q_LOW128 = Q % (1 << 128)


def words(x):
    return [(x >> (32 * i)) & M32 for i in range(8)]


def from_words(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def carries(a, b, sub=False):
    """carry (borrow) out of each of the eight 32-bit words of a + b (a - b): what one chain of sp_chain2 leaves in its SGPR pair"""
    c, out = 0, []
    for x, y in zip(words(a), words(b)):
        t = x - y - c if sub else x + y + c
        c = 1 if (t < 0 or t > M32) else 0
        out.append(c)
    return out


# ------------------------------------------------------------------ integer models
def mont_m(a, b):
    """the eight reduction words m_0..m_7 of the word-by-word Montgomery multiplication, as one integer: -ab/q mod 2^256"""
    return (a * b % W256) * QINV256 % W256


def mont_t(a, b):
    """value before the final conditional subtraction: (ab + mq) / 2^256, in [0, 2q)"""
    t, rem = divmod(a * b + mont_m(a, b) * Q, W256)
    assert rem == 0 and t < 2 * Q
    return t


def fp_add_raw_model(a, b):
    """the exact limbs fp_add returns (host and device forms agree limb for limb): wrap by +38, a second wrap adds 38 to limb 0"""
    s = a + b
    if s < W256:
        return s
    s = s - W256 + 38
    if s >= W256:
        s = s - W256 + 38
    return s


def fp_sub_raw_model(a, b):
    d = a - b
    if d >= 0:
        return d
    d = d + W256 - 38
    if d < 0:
        d = d + W256 - 38
    return d


def fp_fold(a, b):
    """fp_mul's folds: N = lo + 38 hi, c = N >> 256 (the carry word), second = ((N mod 2^256) + 38 c >= 2^256)"""
    hi, lo = divmod(a * b, W256)
    N = lo + 38 * hi
    c = N >> 256
    return c, (N % W256) + 38 * c >= W256


# ristretto255 over affine twisted-Edwards coordinates (RFC 9496 section 4), independent of the extended-coordinate code under test
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)


def _neg(x):
    return x % P & 1


def _abs(x):
    x %= P
    return P - x if x & 1 else x


def sqrt_ratio_m1(u, v):
    u %= P; v %= P
    r = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct, flipped, flipped_i = check == u, check == (-u) % P, check == (-u * SQRT_M1) % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return correct or flipped, _abs(r)


INVSQRT_A_MINUS_D = sqrt_ratio_m1(1, -1 - D)[1]
_DEC, _ENC = {}, {}


def pt_decode(s):
    """encoding (int) -> affine (x, y), or None where RFC 9496 4.3.1 rejects"""
    if s in _DEC:
        return _DEC[s]
    out = None
    if s < P and not s & 1:
        ss = s * s % P
        u1, u2 = (1 - ss) % P, (1 + ss) % P
        u2s = u2 * u2 % P
        v = (-(D * u1 * u1) - u2s) % P
        ok, inv = sqrt_ratio_m1(1, v * u2s)
        den_x = inv * u2 % P
        den_y = inv * den_x * v % P
        x = _abs(2 * s * den_x)
        y = u1 * den_y % P
        if ok and not _neg(x * y) and y != 0:
            out = (x, y)
    _DEC[s] = out
    return out


def pt_encode(pt):
    if pt in _ENC:
        return _ENC[pt]
    x, y = pt
    t = x * y % P
    u1, u2 = (1 + y) * (1 - y) % P, t
    inv = sqrt_ratio_m1(1, u1 * u2 * u2)[1]
    den1, den2 = inv * u1 % P, inv * u2 % P
    z_inv = den1 * den2 * t % P
    if _neg(t * z_inv):
        x, y, den_inv = y * SQRT_M1 % P, x * SQRT_M1 % P, den1 * INVSQRT_A_MINUS_D % P
    else:
        den_inv = den2
    if _neg(x * z_inv):
        y = (-y) % P
    s = _abs(den_inv * (1 - y))
    _ENC[pt] = s
    return s


def pt_add_affine(p, q):
    (x1, y1), (x2, y2) = p, q
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P)


def pt_neg_affine(p):
    return ((-p[0]) % P, p[1])


def pt_mul_affine(k, p):
    acc = (0, 1)
    while k:
        if k & 1:
            acc = pt_add_affine(acc, p)
        p = pt_add_affine(p, p)
        k >>= 1
    return acc


def _pt2(f):
    def g(a, b):
        p, q = pt_decode(a), pt_decode(b)
        return BAD if p is None or q is None else pt_encode(f(p, q))
    return g


def _pt1(f):
    def g(a, b):
        p = pt_decode(a)
        return BAD if p is None else pt_encode(f(p))
    return g


# name -> (family, operation of the other lanes in divergent mode (checkops.hpp CHK_OPS), model(a, b) -> int)
OPS = {
    "fq_add": ("fq", "fq_sub", lambda a, b: (a + b) % Q),
    "fq_sub": ("fq", "fq_add", lambda a, b: (a - b) % Q),
    "fq_neg": ("fq", "fq_dbl", lambda a, b: (-a) % Q),
    "fq_dbl": ("fq", "fq_neg", lambda a, b: 2 * a % Q),
    "fq_mul": ("fq", "fq_add", lambda a, b: a * b * RINV % Q),
    "fq_sqr": ("fq", "fq_dbl", lambda a, b: a * a * RINV % Q),
    "fq_from_mont": ("fq", "fq_neg", lambda a, b: a * RINV % Q),
    "fq_to_mont": ("fq", "fq_dbl", lambda a, b: a * R % Q),
    "fq_invert": ("fq", "fq_sqr", lambda a, b: pow(a, Q - 2, Q) * R2 % Q),
    "fp_add": ("fp", "fp_sub", lambda a, b: (a + b) % P),
    "fp_sub": ("fp", "fp_add", lambda a, b: (a - b) % P),
    "fp_neg": ("fp", "fp_sqr", lambda a, b: (-a) % P),
    "fp_mul": ("fp", "fp_sub", lambda a, b: a * b % P),
    "fp_sqr": ("fp", "fp_neg", lambda a, b: a * a % P),
    "fp_invert": ("fp", "fp_sqr", lambda a, b: pow(a, P - 2, P)),
    "fp_pow_p58_serial": ("fp", "fp_mul", lambda a, b: pow(a, (P - 5) // 8, P)),
    "fp_add_raw": ("fp", "fp_sub_raw", fp_add_raw_model),
    "fp_sub_raw": ("fp", "fp_add_raw", fp_sub_raw_model),
    "pt_recompress": ("pt", "pt_dbl", _pt1(lambda p: p)),
    "pt_add": ("pt", "pt_dbl", _pt2(pt_add_affine)),
    "pt_dbl": ("pt", "pt_add", _pt1(lambda p: pt_add_affine(p, p))),
    "pt_madd0": ("pt", "pt_madd1", _pt2(pt_add_affine)),
    "pt_madd1": ("pt", "pt_madd0", _pt2(lambda p, q: pt_add_affine(p, pt_neg_affine(q)))),
    "pt_compress_z": ("pt", "pt_recompress", _pt1(lambda p: p)),
}
_MEMO = {}


def expect(op, a, b):
    k = (op, a, b)
    if k not in _MEMO:
        _MEMO[k] = OPS[op][2](a, b)
    return _MEMO[k]


# ------------------------------------------------------------------ vector classes
def _search(gen, pred, count, limit=2000000):
    out = []
    for _ in range(limit):
        v = gen()
        if pred(*v):
            out.append(v)
            if len(out) == count:
                return out
    raise AssertionError("search exhausted: %d of %d" % (len(out), count))


def _split(rng, s, bound):
    """(a, b) with a + b = s and a, b < bound"""
    a = rng.randrange(max(0, s - (bound - 1)), min(bound - 1, s) + 1)
    return (a, s - a)


def _ffff_word_classes(rng, C, PRED, bound, positions, prefix):
    """sums whose word k is 0xffffffff before a carry arrives from word k-1 (the carry then runs through it); k = 0 has no carry-in: the
    plain all-ones word. And the mirror for subtraction: equal words k with a borrow arriving (the difference word turns 0xffffffff)."""
    for k in positions:
        def gen(k=k):
            a, b = words(rng.randrange(bound)), words(rng.randrange(bound))
            b[k] = M32 - a[k]
            if k:
                b[k - 1] = rng.randrange(M32 + 1 - a[k - 1], M32 + 1) if a[k - 1] else b[k - 1]
            return (from_words(a), from_words(b))
        pred = (lambda a, b, k=k: a < bound and b < bound and (words(a)[k] + words(b)[k]) == M32 and (k == 0 or carries(a, b)[k - 1] == 1))
        C["%ssum_ffff_carry_w%d" % (prefix, k)] = _search(gen, pred, 4)
        PRED["%ssum_ffff_carry_w%d" % (prefix, k)] = pred
    for k in range(1, 8):
        def gen(k=k):
            a, b = words(rng.randrange(bound)), words(rng.randrange(bound))
            b[k] = a[k]
            b[k - 1] = rng.randrange(a[k - 1] + 1, M32 + 1) if a[k - 1] < M32 else b[k - 1]
            return (from_words(a), from_words(b))
        pred = (lambda a, b, k=k: a < bound and b < bound and words(a)[k] == words(b)[k] and carries(a, b, True)[k - 1] == 1)
        C["%sdiff_zero_borrow_w%d" % (prefix, k)] = _search(gen, pred, 4)
        PRED["%sdiff_zero_borrow_w%d" % (prefix, k)] = pred


def check_classes(C, PRED, bound=None):
    for name, vs in C.items():
        assert len(vs) > 0, name
        for a, b in vs:
            assert 0 <= a < W256 and 0 <= b < W256, name
            if bound is not None:
                assert a < bound and b < bound, name
            assert PRED[name](a, b), (name, hex(a), hex(b))


def fq_addsub_classes(seed=101):
    rng = random.Random(seed)
    C, PRED = {}, {}
    for name, s in (("sum_q-1", Q - 1), ("sum_q", Q), ("sum_q+1", Q + 1)):
        C[name] = [_split(rng, s, Q) for _ in range(8)]
        PRED[name] = lambda a, b, s=s: a + b == s
    C["both_q-1"] = [(Q - 1, Q - 1)]
    PRED["both_q-1"] = lambda a, b: a == b == Q - 1
    C["a_zero"] = [(0, 0), (0, 1), (0, Q - 1)] + [(0, rng.randrange(Q)) for _ in range(5)]
    PRED["a_zero"] = lambda a, b: a == 0
    _ffff_word_classes(rng, C, PRED, Q, range(7), "")
    # s - q borrows out of word 3 and ripples through the zero words 4..6 of q; word 7 then decides (both outcomes present)
    tops = [0x10000000, 0x10000001, 0x1fffffff, 0x0fffffff, 5, 0x10000000, 0x10000001]
    C["sum_minus_q_borrow_w4-6"] = [_split(rng, (t << 224) | rng.randrange(Q_LOW128), Q) for t in tops]
    PRED["sum_minus_q_borrow_w4-6"] = lambda a, b: words(a + b)[4:7] == [0, 0, 0] and carries(a + b, Q, True)[3:7] == [1, 1, 1, 1]
    assert {a + b >= Q for a, b in C["sum_minus_q_borrow_w4-6"]} == {True, False}
    xs = [rng.randrange(1, Q - 1) for _ in range(5)]
    C["diff_0"] = [(0, 0), (Q - 1, Q - 1)] + [(x, x) for x in xs]
    PRED["diff_0"] = lambda a, b: a == b
    C["diff_-1"] = [(0, 1), (Q - 2, Q - 1)] + [(x, x + 1) for x in xs]
    PRED["diff_-1"] = lambda a, b: a - b == -1
    C["diff_+1"] = [(1, 0), (Q - 1, Q - 2)] + [(x + 1, x) for x in xs]
    PRED["diff_+1"] = lambda a, b: a - b == 1
    C["0_minus_q-1"] = [(0, Q - 1)]
    PRED["0_minus_q-1"] = lambda a, b: a == 0 and b == Q - 1

    def gen_borrow_all():
        b = words(rng.randrange(Q))
        a = [rng.randrange(b[0]) if b[0] else 0] + [rng.randrange(b[k] + 1) for k in range(1, 8)]
        return (from_words(a), from_words(b))
    PRED["diff_borrow_all8"] = lambda a, b: carries(a, b, True) == [1] * 8
    C["diff_borrow_all8"] = _search(gen_borrow_all, PRED["diff_borrow_all8"], 8)

    def gen_dq():
        qw = words(Q)
        d_low = from_words([rng.randrange(M32 + 1 - qw[k], M32 + 1) for k in range(4)] + [0] * 4)
        e = (1 << 128) - d_low          # b - a; d = a - b + 2^256 = 2^256 - e has words 4..7 all ones
        b = rng.randrange(e, Q)
        return (b - e, b)
    PRED["diff_plus_q_carry_all8"] = lambda a, b: a < b and carries(a - b + W256, Q) == [1] * 8
    C["diff_plus_q_carry_all8"] = _search(gen_dq, PRED["diff_plus_q_carry_all8"], 8)
    check_classes(C, PRED, Q)
    return C, PRED


def fq_special_operands(seed=102):
    rng = random.Random(seed)
    S = [0, 1, R, R2, Q - 1, Q - 2, 2**252 - 1, 2**252, (Q - 1) // 2]
    for k in range(7):   # 0xffffffff at word k, value kept below q (word 7 of a reduced operand is at most 0x10000000)
        w = words(rng.randrange(1 << 252))
        w[k] = M32
        S.append(from_words(w))
    assert all(x < Q for x in S)
    return S


def fq_mul_classes(seed=103):
    rng = random.Random(seed)
    C, PRED = {}, {}
    S = fq_special_operands()
    C["special_pairs"] = [(a, b) for a in S for b in S]
    PRED["special_pairs"] = lambda a, b: a in S and b in S
    PRED["t_in_[q,2q)"] = lambda a, b: Q <= mont_t(a, b) < 2 * Q
    near = lambda: Q - 1 - rng.randrange(1 << 64)
    C["t_in_[q,2q)"] = (_search(lambda: (rng.randrange(Q), rng.randrange(Q)), PRED["t_in_[q,2q)"], 160)
                        + _search(lambda: (near(), near()), PRED["t_in_[q,2q)"], 128))
    assert not any(mont_t(a, b) == Q for a, b in C["special_pairs"] + C["t_in_[q,2q)"])   # t = q is unreachable (module docstring)
    for i in range(8):
        for tag, val in (("zero", 0), ("ones", M32)):
            def gen(i=i, val=val):
                m = words(rng.getrandbits(256))
                m[i] = val
                b = rng.randrange(Q) | 1
                return ((-from_words(m) * Q) * pow(b, -1, W256) % W256, b)   # ab = -mq mod 2^256
            name = "m%d_%s" % (i, tag)
            PRED[name] = lambda a, b, i=i, val=val: a < Q and b < Q and words(mont_m(a, b))[i] == val
            C[name] = _search(gen, PRED[name], 4)
    check_classes(C, PRED, Q)
    return C, PRED


FP_SPECIAL = [0, 1, 19, 38, P - 1, P, P + 1, 2**255 - 1, 2**255, 2 * P, 2 * P + 37, W256 - 1]


def fp_sqrt(r):
    x = pow(r, (P + 3) // 8, P)
    if x * x % P != r % P:
        x = x * SQRT_M1 % P
    return x if x * x % P == r % P else None


def fp_classes(seed=104):
    rng = random.Random(seed)
    C, PRED = {}, {}
    rr = lambda: rng.getrandbits(256)
    # ---- add
    for name, s in (("sum_2^256-1", W256 - 1), ("sum_2^256", W256), ("sum_2^256+1", W256 + 1)):
        C[name] = [_split(rng, s, W256) for _ in range(8)]
        PRED[name] = lambda a, b, s=s: a + b == s
    C["add_second_wrap"] = [(W256 - 1, W256 - 1)] + [(W256 - 1 - j, W256 - 1 - (k - j)) for k in range(1, 37, 5) for j in (0, k // 2, k)]
    PRED["add_second_wrap"] = lambda a, b: a + b >= 2 * W256 - 38
    assert fp_add_raw_model(W256 - 1, W256 - 1) == 74
    C["add_nowrap_top38"] = [_split(rng, W256 - 1 - k, W256) for k in (0, 1, 17, 36, 37)]
    PRED["add_nowrap_top38"] = lambda a, b: W256 - 38 <= a + b < W256     # the +38 chain carries out (cB) while a + b does not (cA)
    _ffff_word_classes(rng, C, PRED, W256, range(8), "")
    # ---- sub
    xs = [rr() for _ in range(5)]
    C["sub_equal"] = [(0, 0), (W256 - 1, W256 - 1), (P, P)] + [(x, x) for x in xs]
    PRED["sub_equal"] = lambda a, b: a == b
    C["sub_-1"] = [(0, 1), (W256 - 2, W256 - 1)] + [(x, x + 1) for x in xs if x + 1 < W256]
    PRED["sub_-1"] = lambda a, b: a - b == -1
    C["sub_second_borrow"] = [(x, x + e) for e in (W256 - 37, W256 - 1, W256 - 20) for x in (0, 1, 5) if x + e < W256]
    C["sub_second_borrow"] += [(0, W256 - 37), (36, W256 - 1), (0, W256 - 1)]
    PRED["sub_second_borrow"] = lambda a, b: a < b and a - b + W256 < 38
    C["sub_0_minus_x"] = [(0, x) for x in (0, 1, 37, 38, 39, P, W256 - 1)]
    PRED["sub_0_minus_x"] = lambda a, b: a == 0 and b in (0, 1, 37, 38, 39, P, W256 - 1)

    def gen_borrow_all():
        b = words(rr())
        a = [rng.randrange(b[0]) if b[0] else 0] + [rng.randrange(b[k] + 1) for k in range(1, 8)]
        return (from_words(a), from_words(b))
    PRED["sub_borrow_all8"] = lambda a, b: carries(a, b, True) == [1] * 8
    C["sub_borrow_all8"] = _search(gen_borrow_all, PRED["sub_borrow_all8"], 8)
    # ---- mul / sqr
    C["mul_special_pairs"] = [(a, b) for a in FP_SPECIAL for b in FP_SPECIAL]
    PRED["mul_special_pairs"] = lambda a, b: a in FP_SPECIAL and b in FP_SPECIAL
    PRED["mul_fold1_c>=1"] = lambda a, b: fp_fold(a, b)[0] >= 1
    C["mul_fold1_c>=1"] = _search(lambda: (rr(), rr()), PRED["mul_fold1_c>=1"], 32)
    PRED["mul_fold1_c37"] = lambda a, b: fp_fold(a, b)[0] == 37
    C["mul_fold1_c37"] = [(W256 - 1, W256 - 1)] + _search(lambda: (W256 - 1 - rng.randrange(64), W256 - 1 - rng.randrange(64)), PRED["mul_fold1_c37"], 7)
    PRED["mul_fold1_cmax38"] = lambda a, b: fp_fold(a, b)[0] == 38
    C["mul_fold1_cmax38"] = _search(lambda: (W256 - 1 - rng.randrange(1 << 20), W256 - 1 - rng.randrange(1 << 20)), PRED["mul_fold1_cmax38"], 16)
    assert max(fp_fold(a, b)[0] for vs in C.values() for a, b in vs) == 38

    def gen_fold2():
        r, b = rng.randrange(38, 76), rr()
        if b % P == 0:
            b = 1
        a = r * pow(b % P, P - 2, P) % P
        a += P * rng.randrange(0, (W256 - 1 - a) // P + 1)
        return (a, b)
    PRED["mul_second_fold"] = lambda a, b: fp_fold(a, b)[1]
    C["mul_second_fold"] = _search(gen_fold2, PRED["mul_second_fold"], 288)
    sq = []
    for r in range(38, 2000):
        x = fp_sqrt(r)
        if x is None:
            continue
        for a in (x, P - x, x + P, 2 * P - x):
            if a < W256 and fp_fold(a, a)[1]:
                sq.append((a, a))
    C["sqr_second_fold"] = sq
    PRED["sqr_second_fold"] = lambda a, b: a == b and fp_fold(a, a)[1]
    check_classes(C, PRED)
    return C, PRED


_PT_POOL = {}


def pt_material():
    """basepoint multiples 0..15 (encodings computed by the affine model; the CPU test pins them to RFC 9496 A.1), their negations, 64
    generic points and the invalid encodings of RFC 9496 (tests/test_oracle_pins.py)"""
    if _PT_POOL:
        return _PT_POOL
    # the RFC 9496 constants live in a test module of the suite (the one place they are typed in, checked there against libsodium):
    # importing them imports that module
    from tests.test_oracle_pins import BASEPOINT, RFC_BAD
    Bp = pt_decode(int.from_bytes(bytes.fromhex(BASEPOINT), "little"))
    assert Bp is not None
    mult, acc = [], (0, 1)
    for _ in range(16):
        mult.append(acc)
        acc = pt_add_affine(acc, Bp)
    rng = random.Random(105)
    g1, g2 = pt_mul_affine(rng.randrange(Q), Bp), pt_mul_affine(rng.randrange(Q), Bp)
    generic, acc = [], g1
    for _ in range(64):
        generic.append(acc)
        acc = pt_add_affine(acc, g2)
    _PT_POOL.update(mult=mult, generic=generic, bad=[int.from_bytes(bytes.fromhex(h), "little") for h in RFC_BAD])
    return _PT_POOL


def pt_classes():
    m = pt_material()
    enc, mult, gen, bad = pt_encode, m["mult"], m["generic"], m["bad"]
    assert len(bad) == 29 and all(pt_decode(x) is None for x in bad)
    E = [enc(p) for p in mult]
    B = E[1]
    C, PRED = {}, {}
    valid = lambda x: pt_decode(x) is not None
    C["identity"] = [(0, 0), (0, B), (B, 0)]
    PRED["identity"] = lambda a, b: a == 0 or b == 0
    C["small_multiples"] = [(E[k], E[k + 1]) for k in range(15)]
    PRED["small_multiples"] = lambda a, b: a in E and b in E
    C["rfc_multiples"] = [(E[k], E[(3 * k + 1) % 16]) for k in range(16)]
    PRED["rfc_multiples"] = PRED["small_multiples"]
    some = mult[1:9] + gen[:8]
    C["p_plus_neg_p"] = [(enc(p), enc(pt_neg_affine(p))) for p in some]       # pt_madd with the negated entry of P as well
    PRED["p_plus_neg_p"] = lambda a, b: expect("pt_add", a, b) == 0 and a != 0
    C["p_plus_p"] = [(enc(p), enc(p)) for p in some]                           # pt_add on equal operands; pt_madd of P with its own entry
    PRED["p_plus_p"] = lambda a, b: a == b and valid(a) and a != 0
    C["bad_a"] = [(x, B) for x in bad]
    PRED["bad_a"] = lambda a, b: not valid(a) and valid(b)
    C["bad_b"] = [(enc(gen[i]), x) for i, x in enumerate(bad)]
    PRED["bad_b"] = lambda a, b: valid(a) and not valid(b)
    check_classes(C, PRED)
    return C, PRED


def fillers(family, n=128, seed=106):
    rng = random.Random(seed)
    if family == "fq":
        return [(rng.randrange(Q), rng.randrange(Q)) for _ in range(n)]
    if family == "fp":
        return [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(n)]
    g = [pt_encode(p) for p in pt_material()["generic"]]
    return [(g[rng.randrange(64)], g[rng.randrange(64)]) for _ in range(n)]


_FAM = {}


def family_classes(family):
    if family not in _FAM:
        if family == "fq":
            C, PRED = fq_addsub_classes()
            C2, P2 = fq_mul_classes()
            C.update(C2); PRED.update(P2)
        elif family == "fp":
            C, PRED = fp_classes()
        else:
            C, PRED = pt_classes()
        _FAM[family] = (C, PRED)
    return _FAM[family]


# ------------------------------------------------------------------ lane layouts: lists of (class name, a, b), element i = lane i % 64 of wavefront i // 64
LANES_B = (0, 1, 31, 32, 33, 62, 63)
SIZES_D = (1, 63, 64, 65, 255, 257)
PATTERNS_E = (0x5555555555555555, 0x00000000ffffffff, 1, 1 << 63)


def layout_a(family, seed=107):
    """every vector of every class shuffled together with as many uniform random fillers: neighbouring lanes differ"""
    C, _ = family_classes(family)
    rng = random.Random(seed)
    v = [(name, a, b) for name, vs in C.items() for a, b in vs]
    fill = fillers(family)
    v += [("filler", *fill[rng.randrange(len(fill))]) for _ in range(len(v))]
    rng.shuffle(v)
    return v


def layout_b(family, seed=108):
    """per class and lane position L: one wavefront with an edge vector of the class at lane L among 63 random lanes"""
    C, _ = family_classes(family)
    rng = random.Random(seed)
    fill = fillers(family)
    v = []
    for name, vs in C.items():
        for j, L in enumerate(LANES_B):
            wave = [("filler", *fill[rng.randrange(len(fill))]) for _ in range(64)]
            wave[L] = (name, *vs[j % len(vs)])
            v += wave
    return v


def layout_c(family):
    """per class: a whole wavefront of one and the same edge vector (each class's vectors in turn over the suite: first and last)"""
    C, _ = family_classes(family)
    v = []
    for name, vs in C.items():
        for pick in {0, len(vs) - 1}:
            v += [(name, *vs[pick])] * 64
    return v


def layout_d(family, n, seed=109):
    """the runs of size n (partial wavefronts and blocks): every class appears at every n. n = 1: one run per class. Larger n: one run in
    which three lanes of four hold the classes in turn (a rotation that differs with n) and the fourth a filler, so the first lanes, and the
    lone lanes of the last, partially filled wavefront (element 64 of 65, 256 of 257), hold edge vectors"""
    C, _ = family_classes(family)
    names = list(C)
    if n == 1:
        return [[(name, *C[name][0])] for name in names]
    assert n - n // 4 >= len(names)
    rng = random.Random(seed + n)
    fill = fillers(family)
    run, k = [], 0
    for i in range(n):
        if i % 4 == 3:
            run.append(("filler", *fill[rng.randrange(len(fill))]))
        else:
            name = names[(k + n) % len(names)]
            vs = C[name]
            run.append((name, *vs[(k // len(names) + n) % len(vs)]))
            k += 1
    return [run]


def pack(vals):
    return b"".join(x.to_bytes(32, "little") for x in vals)


def expected(op, vec, mode=0, pattern=0):
    alt = OPS[op][1]
    return [expect(op if (mode == 0 or (pattern >> (i & 63)) & 1) else alt, a, b) for i, (_, a, b) in enumerate(vec)]
