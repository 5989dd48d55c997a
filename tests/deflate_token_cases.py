"""Constructed inputs for the deflate token tests (tests/test_deflate_tokens.py on the CPU, tests/test_gpu_deflate_tokens.py on the device), for the
events of tdefl's lazy parse that the corpus of tests/deflate_corpus.py does not contain. Each is built so that the event follows from the
parser's rules, not found by trying: see the comment at each. Test infrastructure only."""
import random

TILE, GROUP = 512, 2                  # positions a tile, tiles a group of the device parse in the GPU test: 98 tiles and 49 groups a 49999 segment
SEGMENTS = [49999, 32768, 65536]      # as tests/test_gpu_deflate_matches.py


def _literal_then_long(rng):
    """a literal and a match of >= 128 from ONE step: a short match is held at p, and at p + 1 a match of >= 128 starts. X is 200 random
    bytes, a b c three bytes that occur nowhere else. "... abc ... bcX ... abcX": at the second abc the earlier abc matches for its three
    bytes and no further (what follows it is not X), so it is held; one position on, "bcX" matches for 202 bytes: a becomes a literal and
    the long match is taken in the same step."""
    x = bytes(rng.randrange(1, 250) for _ in range(200))
    s = bytes([251, 252, 253])
    pad = lambda k: bytes(rng.randrange(1, 250) for _ in range(k))
    return pad(50) + s + pad(40) + s[1:] + x + pad(30) + s + x + pad(20)


def _free_long(rng):
    """a match of >= 128 taken from a free state: a 300-byte random block repeated after a literal that occurs nowhere else, so that the state
    is free where the repeat starts"""
    x = bytes(rng.randrange(1, 250) for _ in range(300))
    return x + bytes([255]) + x + bytes([254]) + x


def _lazy_chain(rng, n):
    """lazy chains of three and more: text over a four-letter alphabet in which every position has a match and the next position often a
    longer one; a chain's third look-up is held at a length that is often not A[p - 1]'s, which neither table answers"""
    words = [bytes(rng.randrange(4) + 97 for _ in range(rng.randrange(3, 12))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[rng.randrange(len(words))]
        if rng.randrange(5) == 0:
            out.append(rng.randrange(4) + 97)
    return bytes(out[:n])


def _held_at_seams(rng, n):
    """a held match where a segment ends, for every segment length of the GPU test: in random bytes, the ten bytes from each multiple of a
    segment length minus one repeat those 600 bytes earlier — the step at seam - 1 finds a match of ten and holds it, the step at seam,
    which decides about it, belongs to the next segment"""
    data = bytearray(rng.randrange(1, 250) for _ in range(n))
    seams = sorted({k * seg for seg in SEGMENTS for k in range(1, n // seg + 1) if k * seg + 16 < n})
    for p in seams:
        data[p - 1:p + 9] = data[p - 601:p - 591]     # the match starts at seam - 1: found there, held, and met at seam by the next segment
    return bytes(data)


def build():
    """{name: bytes}, each at most 200 000 bytes"""
    rng = random.Random(99)
    cases = {
        "literal+long": _literal_then_long(rng),
        "free-long": _free_long(rng),
        "lazy/70001": _lazy_chain(rng, 70001),
        "held-at-seams/200000": _held_at_seams(rng, 200000),
        "zeros+tail/70000": bytes(69000) + bytes(rng.randrange(256) for _ in range(1000)),   # matches of 258 across every tile and group boundary
    }
    return cases
