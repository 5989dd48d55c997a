"""CPU tests of tdefl's lazy parse restated as walks between the parser's free states (spartan_amd/host/deflate.cc: deflate_tokens_host) and of
the coder fed from its tokens (TokenCoder, zlib_from_tokens): the token list, coded, is byte for byte the stream of the sequential deflater —
which tests/test_host_transcript.py pins against the real miniz — at 16, 128 and 1500 probes on the corpus of tests/deflate_corpus.py and the
constructed inputs of tests/deflate_token_cases.py; expanded, it is the input. Every event of the parse and of the block decisions that the
device parse (tests/test_gpu_deflate_tokens.py compares it with these lists) has to get right occurs in these inputs: counted here, on the
CPU, as conditions on the inputs."""
import ctypes
import numpy as np
import pytest
from tests.helpers import load_oracle, sz
from tests import deflate_corpus as dc
from tests import deflate_token_cases as tc

COUNTERS = ("walks", "lookups", "fallbacks", "free_long", "lit_and_long", "span_tile", "span_group", "seam_held", "tokens", "max_jump")
BLOCKS = ("full", "ratio", "stored", "static")


@pytest.fixture(scope="module")
def H():
    from spartan_amd import prover
    return prover.H


@pytest.fixture(scope="module")
def inputs():
    cases = dict(dc.build(load_oracle()))
    cases.update(tc.build())
    return cases


def host_tokens(H, data, probes, segment=0):
    """(tokens as a ctypes array, their number, {counter: value}) of the host model at the GPU test's tile and group sizes"""
    n = len(data)
    tok = (ctypes.c_uint32 * max(1, n))()
    cnt = (ctypes.c_uint64 * len(COUNTERS))()
    geom = (ctypes.c_size_t * 3)(tc.TILE, tc.GROUP, segment)
    k = H.spz_deflate_tokens_host(dc.u8(data), sz(n), ctypes.c_uint(probes), geom, tok, cnt)
    return tok, k, dict(zip(COUNTERS, cnt))


def from_tokens(H, data, tok, ntok, probes, old=0, piece=0):
    cap = 2 * len(data) + 1024
    out = (ctypes.c_uint8 * cap)()
    blocks = (ctypes.c_uint64 * 4)()
    n = H.spz_zlib_from_tokens(dc.u8(data), sz(len(data)), tok, sz(ntok), ctypes.c_uint(probes), ctypes.c_int(old), sz(piece), out, sz(cap), blocks)
    return bytes(out[:n]), dict(zip(BLOCKS, blocks))


def expand(tok, ntok, n):
    """the bytes a token list stands for"""
    t = np.frombuffer(tok, dtype=np.uint32, count=ntok) if ntok else np.zeros(0, np.uint32)
    assert np.all(t >> 31 == 1)
    ln = (t >> 15) & 0x1FF
    step = np.where(ln == 0, 1, ln).astype(np.int64)
    pos = np.cumsum(step) - step
    assert int(step.sum()) == n
    out = np.zeros(n, np.uint8)
    lit = ln == 0
    out[pos[lit]] = (t[lit] & 0xFF).astype(np.uint8)
    for p, l, d in zip(pos[~lit].tolist(), ln[~lit].tolist(), ((t[~lit] & 0x7FFF) + 1).tolist()):
        assert 3 <= l <= 258 and 1 <= d <= min(p, 32768), (p, l, d)
        if d >= l:
            out[p:p + l] = out[p - d:p - d + l]
        else:                                       # an overlapping copy repeats its last d bytes
            reps = -(-l // d)
            out[p:p + l] = np.tile(out[p - d:p], reps)[:l]
    return out.tobytes()


@pytest.mark.parametrize("probes", dc.PROBES)
def test_tokens_code_to_the_deflaters_bytes_and_expand_to_the_input(H, inputs, probes):
    """zlib_from_tokens(deflate_tokens_host(x)) == zlib_miniz_probes(x), all at once and fed a thousand tokens at a time; the tokens expand to x;
    no jump between two free states is longer than 383 (the bound the device's tiles are sized by)"""
    total = dict.fromkeys(COUNTERS + BLOCKS, 0)
    for name, x in inputs.items():
        tok, k, cnt = host_tokens(H, x, probes)
        want = dc.zlib_probes(H, x, probes)
        got, blocks = from_tokens(H, x, tok, k, probes)
        assert got == want, (name, probes)
        assert from_tokens(H, x, tok, k, probes, piece=1000)[0] == want, (name, probes)
        assert expand(tok, k, len(x)) == x, (name, probes)
        assert cnt["tokens"] == k and cnt["max_jump"] <= 383, (name, cnt)
        for key in COUNTERS:
            total[key] = max(total[key], cnt[key]) if key == "max_jump" else total[key] + cnt[key]
        for key in BLOCKS:
            total[key] += blocks[key]
    print("probes %d: %s" % (probes, total))
    # the events, summed over the inputs: a look-up neither table answers, a match of >= 128 from a free state, a literal and a match of >= 128
    # from one step, a block ended by each rule, a stored and a static block, matches across a tile and across a group boundary
    for key in ("fallbacks", "free_long", "lit_and_long", "full", "ratio", "stored", "static", "span_tile", "span_group"):
        assert total[key] > 0, (key, probes, total)


def test_old_header_and_empty_input(H, inputs):
    x = inputs["shape/2^9"]
    tok, k, _ = host_tokens(H, x, 128)
    z, _ = from_tokens(H, x, tok, k, 128, old=1)
    assert z[:2] == b"\x78\x01" and z == dc.zlib_probes(H, x, 128, 1)
    tok, k, _ = host_tokens(H, b"", 128)
    assert k == 0 and from_tokens(H, b"", tok, 0, 128)[0] == dc.zlib_probes(H, b"", 128)


def test_tokens_do_not_depend_on_the_segment_length_and_seams_meet_held_matches(H, inputs):
    """the walk that crosses a segment's end stops there and hands its state on: the same tokens at every segment length of the GPU test, and
    at each of them at least one (input, segment length) pair enters a segment with a held match"""
    held = dict.fromkeys(tc.SEGMENTS, 0)
    for name in ("held-at-seams/200000", "text/200000", "lazy/70001", "sparse/131077"):
        x = inputs[name]
        whole, k, _ = host_tokens(H, x, 128)
        for seg in tc.SEGMENTS:
            tok, k2, cnt = host_tokens(H, x, 128, segment=seg)
            assert k2 == k and dc.first_difference(tok, whole, k) is None, (name, seg)
            held[seg] += cnt["seam_held"]
    assert all(v > 0 for v in held.values()), held


def test_token_words_are_what_the_header_says(H, inputs):
    """bit 30 is missing exactly on a literal that a match of >= 128 follows from the same step; bit 29 only on literals"""
    x = inputs["literal+long"]
    tok, k, cnt = host_tokens(H, x, 128)
    assert cnt["lit_and_long"] >= 1 and cnt["free_long"] == 0
    t = [tok[i] for i in range(k)]
    for i, w in enumerate(t):
        ln = (w >> 15) & 0x1FF
        if not w & (1 << 30):
            assert ln == 0 and i + 1 < k and ((t[i + 1] >> 15) & 0x1FF) >= 128 and t[i + 1] & (1 << 30), i
        if w & (1 << 29):
            assert ln == 0 and w & (1 << 30), i
    assert host_tokens(H, inputs["free-long"], 128)[2]["free_long"] >= 1
