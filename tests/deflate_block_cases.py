"""Constructed inputs for the deflate block tests (tests/test_deflate_blocks.py on the CPU, tests/test_gpu_deflate_emit.py on the device), for the
events of tdefl's coder that the corpus of tests/deflate_corpus.py and the cases of tests/deflate_token_cases.py do not contain. Each follows
from the coder's rules (spartan_amd/csrc/tdefl_rules.hpp), see the comment at each. Test infrastructure only."""
import random

CHUNK = 256                           # tokens a workgroup of the device emission in the GPU test, its minimum: a 30 000-token block has 118 chunks
SEGMENTS = [49999, 32768, 65536]      # as tests/deflate_token_cases.py


def _random(n, seed):
    return random.Random(seed).randbytes(n)


def _text(n):
    import os
    from tests.helpers import ROOT
    text = open(os.path.join(ROOT, "SURVEY.md"), "rb").read()   # the corpus's text
    return (text * (n // len(text) + 1))[:n]


def build(first_block_end):
    """{name: bytes}, each at most 200 000 bytes. first_block_end(data) -> the input position at which the host model closes the first block
    of `data` (tests/test_deflate_blocks.py: first_block_end)"""
    cases = {}
    # The input ends exactly where a check closes a block (at 128 probes, which first_block_end runs at): random bytes have next to no
    # matches, and those are three or four bytes long, so nearly every token is a literal with a check behind it and the code buffer fills
    # after some 58 200 of them; the tokens before that position do not depend on what follows it (no step there finds a match that the
    # input's end would cut), so the trimmed input closes the same block with its last token and the finish block is empty, hence static.
    # Random bytes do not shrink, so the block before it is stored.
    rnd = _random(120000, 5)
    cases["ends-at-check"] = rnd[:first_block_end(rnd)]
    # A coded block that ends within a byte, followed by a stored block: text, which codes to a bit length that is a multiple of 8 one time in
    # eight, then random bytes. The text keeps the first block's code buffer ahead of the ratio rule, so that block runs on into the random
    # bytes until the buffer is full and is still smaller coded than stored; the block after it is random bytes alone and is stored. Three
    # lengths of text, so that at least one coded block ends off a byte boundary.
    for k, n in enumerate((20000, 30011, 40000)):
        cases["text+random/%d" % n] = _text(n) + _random(80000, 6 + k)
    # One block that spans several segments is the corpus's zeros/200000 at a segment of 32768: 776 matches of 258, one block, seven segments.
    # A block with fewer tokens than one chunk of the emission, after full blocks: random bytes, then a tail of 100 literals.
    cases["short-last-block"] = _random(58248 + 100, 9)
    # ... and a whole input of fewer tokens than a chunk that is a dynamic block (48 bytes or more)
    cases["few-tokens"] = bytes(range(100, 200)) + bytes(range(100, 160))
    return cases
