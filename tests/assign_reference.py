"""Python-integer model of the parse of canonical scalar bytes into an assignment (Assignment::new, src/lib.rs:62-88, over
Scalar::from_bytes / to_bytes, ristretto255.rs:390-431): what sp_table_from_bytes, sp_table_to_bytes, sp_table_check_reduced and the host
parser spz_scalars_from_bytes are compared with, exactly. A 32-byte little-endian string v is canonical when v < q; its Montgomery limbs are
the little-endian 64-bit words of v * 2^256 mod q."""
import random
from tests.helpers import Q, R, RINV

NONE = 2**64 - 1          # report[1] when no entry is refused
Q_LIMBS = [(Q >> (64 * i)) & (2**64 - 1) for i in range(4)]


def _limbs(m):
    return [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]


def from_bytes(buf):
    """32 n bytes -> (flat list of 4 n Montgomery limbs, or None when an entry is refused; number of entries >= q; lowest such index or NONE)"""
    buf = bytes(buf)
    assert len(buf) % 32 == 0
    limbs, count, first = [], 0, NONE
    for k in range(len(buf) // 32):
        v = int.from_bytes(buf[32 * k:32 * k + 32], "little")
        if v >= Q:
            count += 1
            first = min(first, k)
        else:
            limbs += _limbs(v * R % Q)
    return (None if count else limbs), count, first


def to_bytes(limbs):
    """flat list of 4 n reduced Montgomery limbs -> 32 n canonical bytes"""
    out = b""
    for k in range(len(limbs) // 4):
        m = sum(int(limbs[4 * k + i]) << (64 * i) for i in range(4))
        assert m < Q
        out += (m * RINV % Q).to_bytes(32, "little")
    return out


def check_reduced(limbs, off=0, n=None):
    """(count, first) of the stored limbs >= q among entries [off, off + n); first counts from the start of the table"""
    n = len(limbs) // 4 - off if n is None else n
    bad = [k for k in range(off, off + n) if sum(int(limbs[4 * k + i]) << (64 * i) for i in range(4)) >= Q]
    return len(bad), (bad[0] if bad else NONE)


def _with_limb_raised(i):
    l = list(Q_LIMBS); l[i] += 1
    return sum(x << (64 * k) for k, x in enumerate(l))


# Below q. With EDGE_INVALID they decide the comparison at every limb: q - 2^64 differs from q first at limb 1 (below), q - 2 and q - 1 only at
# limb 0; 2^252 - 1 is below at the top limb with every lower limb above q's; 2^252 equals q's top limb and is below at limb 1.
EDGE_VALID = [0, 1, 2**64 - 1, 2**64, 2**128, 2**192, 2**252 - 1, 2**252, Q - 2**64, Q - 2, Q - 1, R, R * R % Q]
# Not below q: equal at every limb (q); above only at limb 0, 1, 2 with the limbs over it equal; above at the top limb with small (2^253), with
# mixed and with saturated lower limbs; q's top limb over lower limbs that are all ones.
EDGE_INVALID = [Q, Q + 1, _with_limb_raised(0), _with_limb_raised(1), _with_limb_raised(2), 2**253, 2**255 - 19, 2**255, 2**256 - 1,
                (Q_LIMBS[3] << 192) | (2**192 - 1)]
assert all(v < Q for v in EDGE_VALID) and all(Q <= v < 2**256 for v in EDGE_INVALID)
assert _with_limb_raised(0) == Q + 1 and len(set(EDGE_VALID)) == len(EDGE_VALID)


def enc(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def valid_values(n, seed):
    """n values below q: EDGE_VALID cycled through the even positions, seeded random values on the odd ones"""
    rng = random.Random(seed)
    return [EDGE_VALID[(k // 2) % len(EDGE_VALID)] if k % 2 == 0 else rng.getrandbits(300) % Q for k in range(n)]
