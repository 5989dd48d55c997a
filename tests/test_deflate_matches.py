"""CPU tests of the deflater's match search restated as one independent item per input position (spartan_amd/host/deflate.cc:
deflate_matches_host, MatchParser, zlib_from_matches): tdefl's parser fed from the tables A (a search that starts from nothing) and B (a search
that has to beat the match found one position earlier) writes exactly the bytes of the sequential deflater — which
tests/test_host_transcript.py pins against the real miniz — at 16, 128 and 1500 probes, on the corpus of tests/deflate_corpus.py. The device
search (tests/test_gpu_deflate_matches.py) is compared with these host tables."""
import ctypes
import pytest
from tests.helpers import load_oracle, real_miniz_zlib, sz
from tests import deflate_corpus as dc


@pytest.fixture(scope="module")
def H():
    from spartan_amd import prover
    return prover.H


@pytest.fixture(scope="module")
def corpus():
    return dc.build(load_oracle())


def _from_matches(H, data, L, A, B, probes, old=0):
    cap = 2 * len(data) + 1024
    out = (ctypes.c_uint8 * cap)()
    stats = (ctypes.c_uint64 * 2)()
    n = H.spz_zlib_from_matches(dc.u8(data), sz(len(data)), L, A, B, ctypes.c_uint(probes), ctypes.c_int(old), out, sz(cap), stats)
    return bytes(out[:n]), stats[0], stats[1]


@pytest.mark.parametrize("probes", dc.PROBES)
def test_parser_over_match_tables_writes_the_deflaters_bytes(H, corpus, probes):
    """zlib_from_matches(deflate_matches_host(c)) == zlib_miniz_probes(c) for every input; at 128 probes also == the real miniz at level 6.
    Lookups that neither table answers (a lazy chain of three or more whose held length is not A[p-1]'s) are searched on the spot: they must
    stay under 1 % of all lookups of the corpus — a condition on the restatement (were it common, the tables would not carry the search),
    not a measurement."""
    lookups = fallbacks = 0
    worst = ("", 0)
    for name, c in corpus.items():
        _, A, B = dc.host_tables(H, c, probes)
        got, lk, fb = _from_matches(H, c, None, A, B, probes)
        assert got == dc.zlib_probes(H, c, probes), (name, probes)
        if probes == 128:
            assert got == real_miniz_zlib(c, 6), name
        assert lk <= max(1, len(c)) and fb <= lk
        lookups += lk; fallbacks += fb
        if fb > worst[1]:
            worst = (name, fb)
    print("probes %d: %d fallbacks of %d lookups (%.3f %%), most in %s: %d" % (probes, fallbacks, lookups, 100.0 * fallbacks / lookups, *worst))
    assert fallbacks * 100 < lookups


def test_links_given_or_computed_and_both_headers(H, corpus):
    """the parser with the caller's links and with links of its own gives the same stream; the old-header variant changes the second byte only"""
    for name in ("text/131077", "period/65536", "shape/2^9", "sparse/65538"):
        c = corpus[name]
        L, A, B = dc.host_tables(H, c, 128, links=True)
        z_given, _, fb = _from_matches(H, c, L, A, B, 128)
        z_own, _, fb2 = _from_matches(H, c, None, A, B, 128)
        assert z_given == z_own == dc.zlib_probes(H, c, 128) and fb == fb2, name
        z_old, _, _ = _from_matches(H, c, L, A, B, 128, old=1)
        assert z_old[:2] == b"\x78\x01" and z_old[2:] == z_given[2:] and z_old == dc.zlib_probes(H, c, 128, 1), name


def test_table_entries_are_what_the_header_says(H, corpus):
    """an entry is dist | len << 16 with 3 <= len <= 258 and 1 <= dist <= 32768 where a match was found, (0, 2) in A where none was; B is 0
    wherever A[p - 1] is no held match; the bytes at the match are equal"""
    c = corpus["text/65537"]
    L, A, B = dc.host_tables(H, c, 128, links=True)
    n = len(c)
    found = 0
    for p in range(n):
        dist, ln = A[p] & 0xFFFF, A[p] >> 16
        if dist == 0:
            assert ln == 2
            continue
        found += 1
        assert 3 <= ln <= min(258, n - p) and 1 <= dist <= min(p, 32768) and c[p:p + ln] == c[p - dist:p - dist + ln], p
        if L[p]:
            assert (p - L[p]) % 65536 >= 1
    assert found > n // 2
    for p in range(1, n):
        da, la = A[p - 1] & 0xFFFF, A[p - 1] >> 16
        held = da != 0 and not (la == 3 and da >= 8192) and ((p - 1) & 32767) != da and la < 128
        if not held:
            assert B[p] == 0, p
        else:
            assert (B[p] >> 16) >= la, p
    assert B[0] == 0
