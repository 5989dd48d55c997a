"""CPU tests of tdefl's coder split as the device runs it (spartan_amd/host/deflate.cc: deflate_blocks_host, BlockPlanner, zlib_from_blocks): the
block records found from prefix sums of token costs by a chain of first-hit searches, then tables, headers and bit offsets from each block's
histogram alone, then every token's bits ORed in at its own offset, give byte for byte the stream of the sequential deflater — which
tests/test_host_transcript.py pins against the real miniz — at 16, 128 and 1500 probes on the corpus of tests/deflate_corpus.py and the
constructed inputs of tests/deflate_token_cases.py and tests/deflate_block_cases.py. Every event of the block decisions that the device coder
(tests/test_gpu_deflate_emit.py compares it with these records) has to get right occurs in these inputs: counted here, on the CPU, as
conditions on the inputs."""
import ctypes
import numpy as np
import pytest
from tests.helpers import load_oracle, sz
from tests import deflate_corpus as dc
from tests import deflate_token_cases as tc
from tests import deflate_block_cases as bc
from tests.test_deflate_tokens import host_tokens

COUNTERS = ("full", "ratio", "empty_final", "seam_open", "max_span", "seam_at_boundary", "max_tokens")
STATS = ("stored", "static", "stored_after_midbyte")
REC, HIST = 6, 320
MAX_TOKENS = 58249


@pytest.fixture(scope="module")
def H():
    from spartan_amd import prover
    return prover.H


def host_blocks(H, tok, ntok, n, segment=0):
    """(records as a numpy array of nb x 6, histograms nb x 320, {counter: value}) of the host model"""
    cap = ntok // 11306 + 4
    rec = (ctypes.c_uint64 * (REC * cap))(); hist = (ctypes.c_uint16 * (HIST * cap))(); cnt = (ctypes.c_uint64 * len(COUNTERS))()
    nb = H.spz_deflate_blocks_host(tok, sz(ntok), sz(n), sz(segment), rec, hist, sz(cap), cnt)
    assert nb >= 1, H.spz_last_error()
    return (np.frombuffer(rec, dtype=np.uint64, count=REC * nb).reshape(nb, REC).copy(),
            np.frombuffer(hist, dtype=np.uint16, count=HIST * nb).reshape(nb, HIST).copy(), dict(zip(COUNTERS, cnt)))


def from_blocks(H, data, rec, hist, tok, probes, old=0):
    cap = 2 * len(data) + 1024
    out = (ctypes.c_uint8 * cap)(); st = (ctypes.c_uint64 * 3)()
    r = np.ascontiguousarray(rec, dtype=np.uint64); h = np.ascontiguousarray(hist, dtype=np.uint16)
    n = H.spz_zlib_from_blocks(r.ctypes.data, h.ctypes.data, sz(len(r)), tok, dc.u8(data), sz(len(data)), ctypes.c_uint(probes), ctypes.c_int(old), out, sz(cap), st)
    assert n > 0, H.spz_last_error()
    return bytes(out[:n]), dict(zip(STATS, st))


def first_block_end(H, data, probes=128):
    """the input position at which the host model closes the first block of `data`"""
    tok, k, _ = host_tokens(H, data, probes)
    rec, _, _ = host_blocks(H, tok, k, len(data))
    return int(rec[0][2])


_INPUTS = {}


def all_inputs(H):
    """{name: bytes}: the corpus and both case files, built once"""
    if not _INPUTS:
        _INPUTS.update(dc.build(load_oracle()))
        _INPUTS.update(tc.build())
        _INPUTS.update(bc.build(lambda x: first_block_end(H, x)))
    return _INPUTS


def coinciding_segments(H, data, probes=128):
    """segment lengths at which a block boundary meets a segment's last token: the first position >= 32768 at which the host model closes
    a block, and that position - 1 and + 1"""
    tok, k, _ = host_tokens(H, data, probes)
    rec, _, _ = host_blocks(H, tok, k, len(data))
    ends = np.cumsum(rec[:-1, 2])
    p = int(ends[ends >= 32768][0])
    return [p - 1, p, p + 1]


@pytest.fixture(scope="module")
def inputs(H):
    return all_inputs(H)


@pytest.mark.parametrize("probes", dc.PROBES)
def test_blocks_code_to_the_deflaters_bytes(H, inputs, probes):
    """zlib_from_blocks(deflate_blocks_host(tokens)) == zlib_miniz_probes(x); no block has more than 58249 tokens; the blocks partition the
    token list and the input"""
    total = dict.fromkeys(COUNTERS + STATS, 0)
    for name, x in inputs.items():
        tok, k, _ = host_tokens(H, x, probes)
        rec, hist, cnt = host_blocks(H, tok, k, len(x))
        got, st = from_blocks(H, x, rec, hist, tok, probes)
        assert got == dc.zlib_probes(H, x, probes), (name, probes)
        assert cnt["max_tokens"] <= MAX_TOKENS and int(rec[:, 1].max()) == cnt["max_tokens"], (name, cnt)
        assert int(rec[:, 1].sum()) == k and int(rec[:, 2].sum()) == len(x) and rec[-1][3] == 3 and np.all(rec[:-1, 3] != 3), name
        assert np.array_equal(rec[:, 0], np.cumsum(rec[:, 1]) - rec[:, 1]), name
        if name == "ends-at-check" and probes == 128:   # the input ends where a check closes a block: the finish block is empty, and static
            assert len(rec) >= 2 and rec[-1][1] == 0 and rec[-2][3] in (1, 2) and cnt["empty_final"] == 1 and st["static"] == 1, (rec, st)
        if name.startswith("text+random"):
            assert st["stored"] >= 1, (name, st)
        for key in COUNTERS:
            total[key] = max(total[key], cnt[key]) if key.startswith("max") else total[key] + cnt[key]
        for key in STATS:
            total[key] += st[key]
    print("probes %d: %s" % (probes, total))
    # the events, summed over the inputs: a block closed by each rule, a stored and a static block, a stored block behind a block that ends
    # within a byte; at 128 probes, which the case was cut at, an input that ends where a check closes a block
    for key in ("full", "ratio", "stored", "static", "stored_after_midbyte") + (("empty_final",) if probes == 128 else ()):
        assert total[key] > 0, (key, probes, total)


def test_old_header_and_empty_input(H, inputs):
    x = inputs["shape/2^9"]
    tok, k, _ = host_tokens(H, x, 128)
    rec, hist, _ = host_blocks(H, tok, k, len(x))
    z, _ = from_blocks(H, x, rec, hist, tok, 128, old=1)
    assert z[:2] == b"\x78\x01" and z == dc.zlib_probes(H, x, 128, 1)
    z, _ = from_blocks(H, x, rec, hist, tok, 128, old=0)
    assert z[:2] == b"\x78\x9c" and z == dc.zlib_probes(H, x, 128, 0)
    tok, k, _ = host_tokens(H, b"", 128)
    rec, hist, cnt = host_blocks(H, tok, 0, 0)
    assert len(rec) == 1 and list(rec[0]) == [0, 0, 0, 3, 0, 0] and cnt["empty_final"] == 1
    for old in (0, 1):
        assert from_blocks(H, b"", rec, hist, tok, 128, old)[0] == dc.zlib_probes(H, b"", 128, old)


def test_block_records_do_not_depend_on_the_segment_length(H, inputs):
    """the same records and histograms however the token list is cut; at every segment length of the GPU test an open block is carried over
    a seam; one block touches three segments or more"""
    carried = dict.fromkeys(bc.SEGMENTS, 0)
    span = 0
    for name in ("zeros/200000", "text/200000", "random/200000", "sparse/131077", "held-at-seams/200000", "text+random/30011", "ends-at-check"):
        x = inputs[name]
        tok, k, _ = host_tokens(H, x, 128)
        whole, whist, _ = host_blocks(H, tok, k, len(x))
        for seg in bc.SEGMENTS:
            rec, hist, cnt = host_blocks(H, tok, k, len(x), segment=seg)
            assert np.array_equal(rec, whole) and np.array_equal(hist, whist), (name, seg)
            carried[seg] += cnt["seam_open"]
            span = max(span, cnt["max_span"])
    assert all(v > 0 for v in carried.values()), carried
    assert span >= 3, span
    tok, k, _ = host_tokens(H, inputs["zeros/200000"], 128)
    assert host_blocks(H, tok, k, 200000, segment=32768)[2]["max_span"] >= 3


def test_a_block_boundary_that_meets_a_segments_last_token(H, inputs):
    """the segment length set to a position at which the host model closes a block: the block's last token is the segment's last, the next
    segment starts with an empty carry; one position less and one more move the seam by a token"""
    for name in ("text/200000", "random/200000", "text+random/30011"):
        x = inputs[name]
        tok, k, _ = host_tokens(H, x, 128)
        whole, whist, _ = host_blocks(H, tok, k, len(x))
        segs = coinciding_segments(H, x)
        assert segs[1] >= 32768
        at = []
        for seg in segs:
            rec, hist, cnt = host_blocks(H, tok, k, len(x), segment=seg)
            assert np.array_equal(rec, whole) and np.array_equal(hist, whist), (name, seg)
            at.append(cnt["seam_at_boundary"])
        assert at[1] > 0, (name, segs, at)
