"""The model of Instance::new (tests/sparse_build_reference.py) against the independent statement of the padding rules in
tests/structured_cases.py, for every structured case, and against hand-written cases of the precedence rules: an index is tested before a
scalar, a bad index hides the scalar of its entry, the lowest failing entry of the first failing matrix decides."""
import pytest
from tests.helpers import Q
from tests import sparse_build_reference as sb
from tests import structured_cases as sc

G = dict(row_limit=4, col_limit=7, col_split=5, col_shift=3, pad_count=0, pad_col=5, num_rows=4, num_cols=16)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_model_agrees_with_the_structured_cases(name):
    case = sc.get(name)
    nc, nv, ni, A, B, C = case[:6]
    ncp, nvp, shift = sc.padded_shape(case)
    assert sb.padded(nc, nv, ni) == (ncp, nvp)
    for m in (A, B, C):
        g = sb.geometry(nc, nv, ni, len(m))
        assert (g["num_rows"], g["num_cols"], g["col_shift"], g["col_split"], g["pad_count"]) == (ncp, 2 * nvp, shift, nv, 0)
        assert not sb.invalid_arguments(len(m), g)
    st, shape, mats = sb.instance_new(nc, nv, ni, A, B, C)
    assert st == "ok" and shape == (ncp, nvp)
    for m, got in zip((A, B, C), mats):
        assert got == [(r, c + shift if c >= nv else c, v) for r, c, v in m]          # the statement of dense_stats' column pick
        assert all(r < ncp and c < 2 * nvp for r, c, _ in got)
    # the shifted entries satisfy the same rows over z = (vars, 0.., 1, inputs, 0..)
    z = list(case[6]) + [0] * (nvp - nv) + [1] + list(case[7]) + [0] * (nvp - 1 - ni)
    assert sb.violated_rows(*mats, z, ncp) == []


def test_padding_rules_at_the_small_ends():
    # lib.rs:143-156 as written: 0 becomes 2 and then, 0usize.next_power_of_two() being 1 and not 0, becomes 1
    assert sb.padded(0, 1, 0) == (1, 1) and sb.padded(1, 1, 0) == (2, 1) and sb.padded(2, 1, 0) == (2, 1) and sb.padded(3, 5, 7) == (4, 8)
    assert sb.padded(37, 100, 7) == (64, 128) and sb.padded(64, 3, 3) == (64, 4)
    # pad entries: only for 0 or 1 constraints, and only up to num_cons_padded (lib.rs:191-195)
    assert sb.geometry(0, 4, 1, 0)["pad_count"] == 1 and sb.geometry(1, 4, 1, 0)["pad_count"] == 2 and sb.geometry(1, 4, 1, 1)["pad_count"] == 1
    assert sb.geometry(1, 4, 1, 2)["pad_count"] == 0 and sb.geometry(1, 4, 1, 9)["pad_count"] == 0 and sb.geometry(2, 4, 1, 0)["pad_count"] == 0
    st, shape, mats = sb.instance_new(1, 3, 1, [(0, 4, 7)], [], [(0, 0, 1), (0, 3, 2), (0, 1, 0)])
    assert st == "ok" and shape == (2, 4)
    assert mats[0] == [(0, 5, 7), (1, 3, 0)]                     # the input moves by 1; the pad entry keeps the caller's num_vars as its column
    assert mats[1] == [(0, 3, 0), (1, 3, 0)]
    assert mats[2] == [(0, 0, 1), (0, 4, 2), (0, 1, 0)]          # more entries than num_cons_padded: no pad entry
    st, k, rep = sb.instance_new(0, 3, 1, [(0, 0, 1)], [], [])   # with no constraint every entry has a bad row
    assert (st, k, rep) == ("InvalidIndex", 0, [1, 0, 0, sb.NONE])
    assert sb.instance_new(0, 3, 1, [], [], [])[2] == [[(0, 3, 0)]] * 3


def test_check_order_within_a_matrix():
    ok = [(0, 0, 1), (3, 6, Q - 1), (1, 4, 0), (2, 5, 5)]
    st, rep, out = sb.build(ok, G)
    assert st == sb.OK and rep == [0, sb.NONE, 0, sb.NONE] and out == [(0, 0, 1), (3, 9, Q - 1), (1, 4, 0), (2, 8, 5)]
    for bad in sb.BAD_SCALARS:
        assert sb.build(ok + [(0, 0, bad)], G)[:2] == (sb.ESCALAR, [0, sb.NONE, 1, 4])
    assert sb.build([(4, 0, 1)], G)[:2] == (sb.EINDEX, [1, 0, 0, sb.NONE])            # row = row_limit
    assert sb.build([(0, 7, 1)], G)[:2] == (sb.EINDEX, [1, 0, 0, sb.NONE])            # col = col_limit
    assert sb.build([(2**32 + 1, 0, 1), (0, 2**32 + 2, 1)], G)[:2] == (sb.EINDEX, [2, 0, 0, sb.NONE])   # not truncated to (1, 0), (0, 2)
    assert sb.build([(0, 0, 1), (4, 0, Q)], G)[:2] == (sb.EINDEX, [1, 1, 0, sb.NONE])  # both in one entry: an index error only
    # a bad scalar at i and a bad index at j > i: the scalar decides, both classes are reported; and the reverse
    assert sb.build([(0, 0, 1), (0, 0, Q), (9, 0, 1), (0, 0, Q + 1)], G)[:2] == (sb.ESCALAR, [1, 2, 2, 1])
    assert sb.build([(0, 9, 1), (0, 0, Q), (9, 0, 1)], G)[:2] == (sb.EINDEX, [2, 0, 1, 1])


def test_error_precedence_across_matrices():
    good = [(0, 0, 1), (1, 1, 2)]
    assert sb.instance_new(2, 2, 0, good + [(1, 0, Q)], [(2, 0, 1)] + good, good) == ("InvalidScalar", 0, [0, sb.NONE, 1, 2])
    assert sb.instance_new(2, 2, 0, good + [(1, 3, 1)], [(0, 0, Q)] + good, good) == ("InvalidIndex", 0, [1, 2, 0, sb.NONE])
    assert sb.instance_new(2, 2, 0, good, good, [(0, 0, 2**256 - 1)]) == ("InvalidScalar", 2, [0, sb.NONE, 1, 0])


def test_invalid_argument_conditions():
    assert not sb.invalid_arguments(3, G) and not sb.invalid_arguments(0, G)
    for change in (dict(num_rows=0), dict(num_cols=0), dict(row_limit=5), dict(col_limit=14), dict(col_shift=10), dict(pad_count=2, num_rows=4),
                   dict(pad_count=1, pad_col=16), dict(num_rows=2**32), dict(num_cols=2**32)):
        assert sb.invalid_arguments(3, dict(G, **change)), change
    assert sb.invalid_arguments(2**32 - 1, G) and sb.invalid_arguments(2**32 - 2, dict(G, pad_count=1)) and not sb.invalid_arguments(2**32 - 2, dict(G, num_rows=2**32 - 1))
    assert not sb.invalid_arguments(3, dict(G, col_limit=13)) and not sb.invalid_arguments(3, dict(G, pad_count=1, pad_col=15))


def test_products_of_a_small_matrix():
    ent = [(0, 1, 2), (1, 0, 3), (0, 1, 5), (1, 2, Q - 1)]                 # (0, 1) twice: the entries add up
    z = [10, 20, 30]
    assert sb.mulvec(ent, z, 2) == [140, 0] and sb.eval_table(ent, [1, 2], 3) == [6, 7, (2 * (Q - 1)) % Q]
    assert sb.evaluate(ent, [1, 2], [3, 4, 5]) == (28 + 18 + 10 * (Q - 1)) % Q
    assert sb.csr_order(ent) == [(0, 1, 2), (0, 1, 5), (1, 0, 3), (1, 2, Q - 1)] and sb.csc_order(ent) == [(1, 0, 3), (0, 1, 2), (0, 1, 5), (1, 2, Q - 1)]
