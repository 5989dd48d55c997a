"""The inputs of the deflate match-table tests (tests/test_deflate_matches.py on the CPU, tests/test_gpu_deflate_matches.py on the device): four
kinds of bytes at the lengths where tdefl's parser or the restated search changes path — nothing, less than one 3-byte hash, the static /
dynamic block threshold (48), the longest match (258), the dictionary (32768) and the 16-bit chain positions (65536) with their neighbours, a
length that is no multiple of anything — plus the real input, bincode(R1CSShape) as the oracle serialises it, and data whose period is the
dictionary size and the chain-position modulus (where a hash head aliases). Test infrastructure only."""
import ctypes, os, random
from tests.helpers import ROOT, sz, vp, oracle_shape_bincode

LENGTHS = [0, 1, 2, 3, 4, 47, 48, 49, 257, 258, 259, 32767, 32768, 32769, 65535, 65536, 65537, 65538, 131077, 200000]
PROBES = [16, 128, 1500]          # miniz levels 4, 6 (Compression::default()), 10
LONGEST = 200000


def _kinds():
    rng = random.Random(2024)
    text = open(os.path.join(ROOT, "SURVEY.md"), "rb").read()
    text = (text * (LONGEST // len(text) + 1))[:LONGEST]
    rnd = rng.randbytes(LONGEST)
    sparse = bytearray(LONGEST)
    for _ in range(LONGEST // 12):   # one byte in twelve is not zero: long zero runs, short literals, many equal hashes
        sparse[rng.randrange(LONGEST)] = rng.randrange(1, 256)
    return {"zeros": bytes(LONGEST), "random": rnd, "text": text, "sparse": bytes(sparse)}


def build(orc):
    """{name: bytes}: 80 + 3 + 2 inputs"""
    cases = {}
    for kind, data in _kinds().items():
        for n in LENGTHS:
            cases["%s/%d" % (kind, n)] = data[:n]
    for s in (4, 9, 12):
        N = 1 << s
        oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(10), ctypes.c_uint64(3)))
        cases["shape/2^%d" % s] = oracle_shape_bincode(orc, oi)
        orc.orc_instance_free(oi)
    rng = random.Random(7)
    for period in (32768, 65536):
        block = bytes(rng.randrange(8) for _ in range(period))   # a small alphabet: every hash has a long chain, in every period the same
        cases["period/%d" % period] = (block * (LONGEST // period + 1))[:LONGEST]
    assert len(cases) == 85
    return cases


def u8(data):
    return (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data) if data else (ctypes.c_uint8 * 1)()


def host_tables(H, data, probes, links=False):
    """(L or None, A, B) as ctypes arrays: the host search (spz_deflate_matches_host)"""
    n = len(data)
    A = (ctypes.c_uint32 * max(1, n))(); B = (ctypes.c_uint32 * max(1, n))()
    L = (ctypes.c_uint16 * max(1, n))() if links else None
    H.spz_deflate_matches_host(u8(data), sz(n), ctypes.c_uint(probes), L, A, B)
    return L, A, B


def zlib_probes(H, data, probes, old=0):
    cap = 2 * len(data) + 1024
    out = (ctypes.c_uint8 * cap)()
    n = H.spz_zlib_probes(u8(data), sz(len(data)), ctypes.c_uint(probes), ctypes.c_int(old), out, sz(cap))
    return bytes(out[:n])


def first_difference(got, want, n):
    """index of the first differing element of two ctypes arrays, or None"""
    if n == 0 or bytes(memoryview(got).cast("B")[:n * ctypes.sizeof(got._type_)]) == bytes(memoryview(want).cast("B")[:n * ctypes.sizeof(want._type_)]):
        return None
    return next(i for i in range(n) if got[i] != want[i])
