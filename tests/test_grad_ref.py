"""The gradient reference (tests/grad_ref.py) against answers worked out by hand, CPU only.

One 3 x 3 case per op: duplicates, an empty row (1), an empty column (2) and a repeated selection.
The forwards are also held against the exact references of tests/reduce_ref.py on a larger case,
and the precondition helpers have to refuse data that breaks them."""
import pytest
import torch

import grad_ref as gr
from reduce_ref import coalesce_ref, group_lengths, segment_ref, spspmm_ref

F64 = torch.float64
# unsorted, (2, 1) and (0, 0) stored twice; row 1 and column 2 hold nothing
INDEX = torch.tensor([[2, 0, 0, 2, 0], [1, 0, 1, 1, 0]])
VALUE = torch.tensor([1.0, 2.0, 3.0, -2.0, -1.0])
# the same matrix coalesced with add, and a second operand
INDEX_A, VALUE_A = torch.tensor([[0, 0, 2], [0, 1, 1]]), torch.tensor([1.0, 3.0, -1.0])
INDEX_B, VALUE_B = torch.tensor([[0, 2], [1, 0]]), torch.tensor([2.0, 4.0])


def t(*x, dtype=torch.float32):
    return torch.tensor(x, dtype=dtype)


def eq(got, want):
    assert got.dtype == want.dtype and torch.equal(got, want), (got, want)


@pytest.mark.parametrize("op,out,grad", [
    ("add", t(1, 3, -1), t(5, 2, -3, 5, 2)),
    ("mean", t(0.5, 3, -0.5), t(2.5, 1, -3, 2.5, 1)),
])
def test_coalesce(op, out, grad):
    index, got, (g,) = gr.coalesce_grad_ref(INDEX, VALUE, 3, 3, op, t(2, -3, 5, dtype=F64))
    assert index.tolist() == [[0, 0, 2], [0, 1, 1]]
    eq(got, out)
    eq(g, grad)


@pytest.mark.parametrize("dim,reduce,coef,out,grad", [
    (1, "sum", t(1, 2, 3, dtype=F64), t(4, 0, -1), t(3, 1, 1, 3, 1)),
    (1, "mean", t(1, 2, 3, dtype=F64), t(4 / 3, 0, -0.5), t(1.5, 1 / 3, 1 / 3, 1.5, 1 / 3)),
    (0, "sum", t(1, 2, 3, dtype=F64), t(1, 2, 0), t(2, 1, 2, 2, 1)),
    (0, "mean", t(1, 2, 3, dtype=F64), t(0.5, 2 / 3, 0), t(2 / 3, 0.5, 2 / 3, 2 / 3, 0.5)),
    (None, "sum", torch.tensor(2.0, dtype=F64), torch.tensor(3.0), t(2, 2, 2, 2, 2)),
    (None, "mean", torch.tensor(2.0, dtype=F64), torch.tensor(0.6), t(0.4, 0.4, 0.4, 0.4, 0.4)),
])
def test_reductions(dim, reduce, coef, out, grad):
    got, (g,) = gr.reduce_grad_ref(INDEX, VALUE, 3, 3, dim, reduce, coef)
    eq(got, out)
    eq(g, grad)


def test_reduction_over_a_value_dim():
    value = torch.tensor([[1.0, 2.0], [3.0, 5.0]])
    index = torch.tensor([[0, 2], [1, 1]])
    got, (g,) = gr.reduce_grad_ref(index, value, 3, 3, 2, "mean", t(2, 4, dtype=F64))
    eq(got, t(1.5, 4))
    eq(g, torch.tensor([[1.0, 1.0], [2.0, 2.0]]))


def test_repeated_selection():
    got, (g,) = gr.select_ref(VALUE, torch.tensor([4, 4, 0]), t(1, 2, 3, dtype=F64))
    eq(got, t(-1, -1, 1))
    eq(g, t(3, 0, 0, 0, 3))


def test_selection_then_mean():
    """Entry 4 is taken twice into group 0 (of four) and once into group 1 (of two): 1 / 4 + 1 / 4 + 3 / 2."""
    sel, group = torch.tensor([4, 4, 0, 1, 4, 2]), torch.tensor([0, 0, 0, 0, 1, 1])
    gr.check_pow2(torch.bincount(group))
    got, (g,) = gr.select_reduce_grad_ref(VALUE, sel, group, 3, "mean", t(1, 3, 8, dtype=F64))
    eq(got, t(0.25, 1, 0))
    eq(g, t(0.25, 0.25, 1.5, 0, 2))


def test_add_and_mul():
    index, got, (ga, gb) = gr.add_grad_ref(INDEX_A, VALUE_A, INDEX_B, VALUE_B, 3, 3, t(1, 2, 3, 4, dtype=F64))
    assert index.tolist() == [[0, 0, 2, 2], [0, 1, 0, 1]]
    eq(got, t(1, 5, 4, -1))
    eq(ga, t(1, 2, 4))
    eq(gb, t(2, 3))
    index, got, (ga, gb) = gr.mul_grad_ref(INDEX_A, VALUE_A, INDEX_B, VALUE_B, 3, 3, t(5, dtype=F64))
    assert index.tolist() == [[0], [1]]
    eq(got, t(6))
    eq(ga, t(0, 10, 0))
    eq(gb, t(15, 0))
    with pytest.raises(AssertionError, match="coalesced"):
        gr.mul_grad_ref(INDEX, VALUE, INDEX_B, VALUE_B, 3, 3)


@pytest.mark.parametrize("reduce,out,grad", [
    ("sum", t(2, 3, 3, -1, -1), t(2, 5, 9)),
    ("mean", t(1, 3, 3, -1, -1), t(1, 5, 9)),
])
def test_to_symmetric(reduce, out, grad):
    index, got, (g,) = gr.symmetric_grad_ref(INDEX_A, VALUE_A, 3, reduce, t(1, 2, 3, 4, 5, dtype=F64))
    assert index.tolist() == [[0, 0, 1, 1, 2], [0, 1, 0, 2, 1]]
    eq(got, out)
    eq(g, grad)


def test_dense_broadcast():
    got, (gv, gw) = gr.broadcast_grad_ref(INDEX_A, VALUE_A, torch.tensor([[2.0], [5.0], [-1.0]]), "mul",
                                          t(1, 2, 3, dtype=F64))
    eq(got, t(2, 6, 1))
    eq(gv, t(2, 4, -3))
    eq(gw, torch.tensor([[7.0], [0.0], [-3.0]]))
    got, (gv, gw) = gr.broadcast_grad_ref(INDEX_A, VALUE_A, torch.tensor([[1.0, 2.0, 3.0]]), "add",
                                          t(1, 2, 3, dtype=F64))
    eq(got, t(2, 5, 1))
    eq(gv, t(1, 2, 3))
    eq(gw, torch.tensor([[1.0, 5.0, 0.0]]))


def test_spspmm():
    index_b, value_b = torch.tensor([[0, 1, 1], [0, 0, 2]]), torch.tensor([2.0, 1.0, -3.0])  # row 2, column 1 empty
    index, got, (ga, gb) = gr.spspmm_grad_ref(INDEX_A, VALUE_A, index_b, value_b, 3, 3, 3, t(1, 2, 3, 4, dtype=F64))
    assert index.tolist() == [[0, 0, 2, 2], [0, 2, 0, 2]]
    eq(got, t(5, -9, -1, 3))
    eq(ga, t(2, -5, -9))
    eq(gb, t(1, 0, 2))
    # an operand without values counts as ones and gets no gradient
    _, got, (ga, gb) = gr.spspmm_grad_ref(INDEX_A, None, index_b, value_b, 3, 3, 3, t(1, 2, 3, 4, dtype=F64))
    eq(got, t(3, -3, 1, -3))
    assert ga is None
    eq(gb, t(1, 4, 6))
    # terms that cancel still make an entry
    index, got, _ = gr.spspmm_grad_ref(torch.tensor([[0, 0], [0, 1]]), t(1, 1), torch.tensor([[0, 1], [0, 0]]), t(1, -1),
                                       1, 2, 1)
    assert index.tolist() == [[0], [0]]
    eq(got, t(0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
def test_forwards_equal_the_exact_references(dtype):
    lengths = torch.as_tensor(group_lengths("edges"))
    nkeys, n = lengths.numel(), 1 << 20
    key = torch.unique(torch.randint(0, 1 << 40, (4 * nkeys,), generator=torch.Generator().manual_seed(4)))[:nkeys]
    key = torch.repeat_interleave(key, lengths)
    shuffle = torch.randperm(key.numel(), generator=torch.Generator().manual_seed(5))
    index = torch.stack([key // n, key % n])[:, shuffle]
    value = gr.values(key.numel(), dtype, (), seed=6)[shuffle]
    gr.check_values(value, gr.VALUE_MAX)
    for op in ("add", "mean"):
        want_i, want_v = coalesce_ref(index, value, n, n, op)
        got_i, got_v, _ = gr.coalesce_grad_ref(index, value, n, n, op)
        assert torch.equal(got_i, want_i)
        eq(got_v, want_v)
    indptr = torch.zeros(nkeys + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lengths, 0)
    rows = torch.repeat_interleave(torch.arange(nkeys), lengths)
    for reduce in ("sum", "mean"):
        got, _ = gr.reduce_grad_ref(torch.stack([rows, rows]), value, nkeys, nkeys, 1, reduce)
        eq(got, segment_ref(value, indptr, reduce))


def test_spspmm_forward_equals_the_exact_reference():
    g = torch.Generator().manual_seed(7)
    m, k, n = 40, 30, 50
    ka = torch.sort(torch.randperm(m * k, generator=g)[:300]).values
    kb = torch.sort(torch.randperm(k * n, generator=g)[:300]).values
    ia, ib = torch.stack([ka // k, ka % k]), torch.stack([kb // n, kb % n])
    va, vb = gr.values(300, torch.float32, (), 8), gr.values(300, torch.float32, (), 9)
    want_i, want_v = spspmm_ref(ia, va, ib, vb, m, k, n)
    got_i, got_v, _ = gr.spspmm_grad_ref(ia, va, ib, vb, m, k, n)
    assert torch.equal(got_i, want_i)
    eq(got_v, want_v)


def test_half_values_keep_their_sums_small():
    for dtype in (torch.float16, torch.bfloat16):
        v = gr.values(5001, dtype, (), 1).double()
        for start in (0, 1):
            assert float(v[start:].sum().abs()) <= 2 * gr.VALUE_MAX


def test_preconditions_refuse_what_breaks_them():
    gr.check_values(t(-3, 0, 3), 3)
    with pytest.raises(AssertionError, match="above"):
        gr.check_values(t(4), 3)
    with pytest.raises(AssertionError, match="non-integer"):
        gr.check_values(t(0.5), 3)
    with pytest.raises(AssertionError, match="-0.0"):
        gr.check_values(t(-0.0), 3)
    with pytest.raises(AssertionError, match="non-finite"):
        gr.check_values(t(float("inf")), 3)
    group = torch.zeros(3, dtype=torch.int64)
    gr.check_sums(t(1 << 22, 1 << 22, 1 << 22, dtype=F64), group, 1, torch.float32)
    with pytest.raises(AssertionError, match="sum"):
        gr.check_sums(t(1 << 23, 1 << 23, 1, dtype=F64), group, 1, torch.float32)
    gr.check_sums(t(1 << 23, 1 << 23, 1, dtype=F64), group, 1, torch.float64)
    with pytest.raises(AssertionError, match="not every such integer"):
        gr.check_sums(t(200, 57, 0, dtype=F64), group, 1, torch.bfloat16)
    gr.check_sums(t(200, 57, 0, dtype=F64), group, 1, torch.float16)
    gr.check_pow2(torch.tensor([0, 1, 2, 64, 4096]))
    with pytest.raises(AssertionError, match="power-of-two"):
        gr.check_pow2(torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="min / max"):
        gr.coalesce_grad_ref(INDEX, VALUE, 3, 3, "max")
