"""CPU checks of tests/eval_many_reference.py: the half-table identity against chi_at, the model of the batched evaluation against a direct
multilinear evaluation of a tiny dense matrix, and the case lists of tests/test_gpu_eval_many.py against the dispatch they are meant to hit."""
import random
from tests import eval_many_reference as E
from tests import fq_reference as F
from tests import field_vectors as V
from tests.helpers import Q, R, RINV


def _point(rng, ell, edges):
    return [edges[rng.randrange(len(edges))] if rng.random() < 0.4 else rng.randrange(Q) for _ in range(ell)]


def test_half_table_identity_against_chi_at():
    rng = random.Random(41)
    edges = V.fq_special_operands()
    for ell in (1, 2, 3, 8, 9, 13, 14, 17):
        hi, lo = E.split(ell)
        assert hi + lo == ell and 0 <= hi - lo <= 1 and hi <= 16
        for trial in range(2):
            r = _point(rng, ell, edges if trial else [rng.randrange(Q)])
            H, L = E.half_tables(r)
            assert len(H) == 1 << hi and len(L) == 1 << lo
            full = F.chi(r)
            assert full == [F.mm(h, l) for h in H for l in L]                     # i = (i >> lo) 2^lo + (i & mask): hi-major
            n = 1 << ell
            for i in {0, 1, n - 1, n // 2, (1 << lo) - 1, (1 << lo) % n, rng.randrange(n), rng.randrange(n)}:
                assert E.chi_from_halves(r, i) == F.chi_at(r, i) == full[i], (ell, i)
    assert E.half_tables([5])[1] == [F.ONE]                                        # lo = 0: the one-entry table


def test_model_against_a_direct_multilinear_evaluation():
    rng = random.Random(42)
    for ex, ey in ((1, 1), (1, 2), (2, 3), (3, 2)):
        nr, nc = 1 << ex, 1 << ey
        dense = [[rng.randrange(Q) if rng.random() < 0.7 else 0 for _ in range(nc)] for _ in range(nr)]      # field values
        # as entries, with one value split over two entries of the same (row, col)
        ent = [(i, j, dense[i][j] * R % Q) for i in range(nr) for j in range(nc) if dense[i][j]]
        i, j, v = ent[0]
        part = rng.randrange(Q)
        ent = [(i, j, part), (i, j, (v - part) % Q)] + ent[1:]
        rng.shuffle(ent)
        rxs = [[rng.randrange(Q) for _ in range(ex)] for _ in range(3)] + [[0] * ex, [F.ONE] * ex]
        rys = [[rng.randrange(Q) for _ in range(ey)] for _ in range(3)] + [[F.ONE] * ey, [0] * ey]
        got = E.evaluate_many([ent, []], rxs, rys)
        for k, (rx, ry) in enumerate(zip(rxs, rys)):
            want = E.dense_mle(dense, [x * RINV % Q for x in rx], [y * RINV % Q for y in ry])
            assert got[k][0] * RINV % Q == want and got[k][1] == 0
        # a point of the hypercube picks the entry
        assert got[3][0] * RINV % Q == dense[0][nc - 1] and got[4][0] * RINV % Q == dense[nr - 1][0]


def test_case_lists_sit_on_the_dispatch_boundaries():
    cap = E.partials_cap()
    assert cap == 1024
    assert {E.padded(K) for K in E.KS} == {1, 2, 4, 8, 64} and sum(E.padded(K) != K for K in E.KS) >= 4
    assert max(E.KS) == E.MAX_K
    for K in (1, 3, 64):
        at, past = E.nnz_at_cap(K)
        assert E.blocks(at - 1, K) == cap - 1 and E.blocks(at, K) == cap and E.blocks(past, K) == cap
        assert past * E.padded(K) > cap * 256                                      # a second grid-stride pass
    assert E.blocks(0, 1) == 1 and E.blocks(256, 1) == 1 and E.blocks(257, 1) == 2    # 255, 256, 257 straddle the first block at Kp = 1
    assert {e // 2 for pair in E.ELLS for e in pair} >= {0, 1, 4, 6, 7} and any(a != b for a, b in E.ELLS)
