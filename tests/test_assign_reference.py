"""The model of tests/assign_reference.py against the oracle's Scalar::from_bytes / to_bytes (orc_fq_from_bytes, orc_fq_to_bytes) and against
tests.helpers.to_mont_limbs: on every edge value and on 1000 seeded random 32-byte strings, valid and invalid alike."""
import ctypes, random
from tests.helpers import Q, u64x4, to_mont_limbs
from tests import assign_reference as ar


def _oracle_parse(orc, b):
    out = u64x4()
    ok = orc.orc_fq_from_bytes(bytes(b), out)
    return ok, list(out)


def _agree(orc, b):
    limbs, count, first = ar.from_bytes(b)
    ok, want = _oracle_parse(orc, b)
    v = int.from_bytes(b, "little")
    assert ok == (1 if v < Q else 0)
    if ok:
        assert (count, first) == (0, ar.NONE) and limbs == want
        back = (ctypes.c_uint8 * 32)()
        orc.orc_fq_to_bytes(u64x4(*want), back)
        assert bytes(back) == b == ar.to_bytes(limbs)
    else:
        assert limbs is None and (count, first) == (1, 0)
    return ok


def test_model_agrees_with_the_oracle_on_every_edge_value(orc):
    for v in ar.EDGE_VALID:
        assert _agree(orc, v.to_bytes(32, "little")) == 1, hex(v)
    for v in ar.EDGE_INVALID:
        assert _agree(orc, v.to_bytes(32, "little")) == 0, hex(v)


def test_model_agrees_with_the_oracle_on_random_strings(orc):
    rng = random.Random(0xa551)
    seen = [0, 0]
    for k in range(1000):
        b = bytes(rng.randrange(256) for _ in range(32))
        if k % 2:                                   # uniform strings are invalid 15 times in 16: every other one gets a top byte below q's
            b = b[:31] + bytes([rng.randrange(0x11)])
        seen[_agree(orc, b)] += 1
    assert min(seen) >= 400


def test_model_agrees_with_to_mont_limbs_and_reports_positions():
    vals = ar.valid_values(200, 7)
    limbs, count, first = ar.from_bytes(ar.enc(vals))
    assert (count, first) == (0, ar.NONE)
    assert limbs == [x for v in vals for x in to_mont_limbs(v)]
    assert ar.to_bytes(limbs) == ar.enc(vals)
    assert ar.check_reduced(limbs) == (0, ar.NONE)
    bad = list(vals); bad[17] = Q; bad[150] = 2**256 - 1
    assert ar.from_bytes(ar.enc(bad)) == (None, 2, 17)
    raw = [x for v in (Q - 1, Q, 2**256 - 1, 0) for x in ar._limbs(v)]
    assert ar.check_reduced(raw) == (2, 1) and ar.check_reduced(raw, 2, 2) == (1, 2) and ar.check_reduced(raw, 3, 1) == (0, ar.NONE)
