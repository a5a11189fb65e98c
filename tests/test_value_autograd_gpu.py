"""Exact forward and gradient of every route a TRACKED value takes.

Where `ops.needs_grad(value)` holds, the call sites leave their fused route (the value riding a sort
as payload, `unique_sorted_reduce`, `coalesce_chain`, `permute_apply`, `merge_sorted` with payloads)
for a differentiable one built from `ops.gather_rows` and `ops.segment_csr`.  Every site gets four
checks (`site`):

  (a) the tracked forward equals the fused forward of the same detached input bit for bit, index and
      value, and both equal the float64 reference (tests/grad_ref.py: dense float64, torch's autograd);
  (b) the gradient of (out * coef).sum() equals the reference's bit for bit;
  (c) a spy on `ops` shows that the tracked call used no fused op, and that the detached call and the
      `torch.no_grad()` call with a requires_grad value did (where the site has one);
  (d) the result requires grad and has a grad_fn (or IS the input, where a shortcut returns it), the
      input is not modified and its `_version` is unchanged.

Data: values in [-3, 3], coefficients and dense operands in [-8, 8]; every test asserts on its own data
that all sums are exact (grad_ref.check_sums), so there are no tolerances.  A mean is one division
per element; where quotients add up (mean after a repeated selection) run lengths are powers of two.
Integer-typed values cannot require grad (torch refuses `requires_grad_()` on them), so the types are
fp32, fp64, fp16 and bf16, and fp32 with trailing dims (1,), (3,), (2, 2) — 4, 12 and 16 bytes a row.
"""
import functools

import numpy as np
import pytest
import torch

import grad_ref as gr
from exact_ref import pow2_degrees
from reduce_ref import HALF_TYPES, coalesce_ref, group_reduce, spspmm_terms

pytestmark = pytest.mark.gpu

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
FUSED = ("sort_pairs", "sort_pairs_field", "unique_sorted_reduce", "coalesce_chain", "permute_apply", "merge_sorted")
KINDS = [(F32, ()), (F64, ()), (F32, (1,)), (F32, (3,)), (F32, (2, 2)), (F16, ()), (BF16, ())]
KIND_IDS = ["f32", "f64", "f32x1", "f32x3", "f32x2x2", "f16", "bf16"]
# run lengths of duplicates / row degrees: 1, 2, around a wave half, a wave, a block, one long run; gaps between
RUNS = [0, 1, 2, 0, 31, 32, 33, 63, 64, 65, 0, 0, 255, 256, 257, 5000, 1, 0]
BIG = 1 << 20  # rows and columns of the wide matrices: keys up to 2^40


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cuda(x):
    return None if x is None else x.cuda()


def scalar4(dtype, tail):
    return dtype == F32 and tail == ()


class Spy:
    """Records (name, args, kwargs) of every call of `ops.<name>` while active."""

    def __init__(self, *names):
        from paddle_sparse_amd import ops

        self.ops, self.names, self.calls = ops, names, []
        self.real = {n: getattr(ops, n) for n in names}

    def __enter__(self):
        for n in self.names:
            setattr(self.ops, n, (lambda n_: lambda *a, **k: self.calls.append((n_, a, k)) or self.real[n_](*a, **k))(n))
        return self

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(self.ops, n, f)

    def used(self):
        """Names called; merge_sorted counts only with payloads (without, it is the tracked route's own merge)."""
        out = set()
        for name, a, k in self.calls:
            if name == "merge_sorted" and (a[2] if len(a) > 2 else k.get("payload_a")) is None:
                continue
            out.add(name)
        return out


def same(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{tuple(got.shape)} for {want.dtype}{tuple(want.shape)}"
    if not torch.equal(got, want):
        diff = (got.double() - want.double()).abs().reshape(-1)
        raise AssertionError(f"{what}: {int((diff > 0).sum())} of {diff.numel()} differ, max |diff| {float(diff.max())} "
                             f"at {int(diff.argmax())}")


def plain_leaf(v):
    return v.clone().requires_grad_(True)


def misaligned_leaf(v):
    """The same values as a contiguous leaf that starts one element into its buffer."""
    flat = torch.empty(v.numel() + 1, dtype=v.dtype, device=v.device)
    flat[1:] = v.reshape(-1)
    leaf = flat[1:].view(v.shape).detach().requires_grad_(True)
    assert leaf.data_ptr() % 16 != 0 and leaf.is_contiguous()
    return leaf


def site(call, operands, ref_out, ref_grads, coef, fused=None, track=None, ref_index=None, leaf_of=plain_leaf,
         forbid=(), detached_uses=()):
    """The four checks.  call(*values) -> (index | None, value) on GPU tensors; operands: CPU tensors (None = no
    values); track: which operands require grad (default all that have values); fused: the fused ops the detached
    route has to use (None: the site has no fused route, nothing asked of the detached call); forbid / detached_uses:
    further ops the tracked forward must not / the detached forward must call."""
    track = track or tuple(v is not None for v in operands)
    names = FUSED + tuple(forbid) + tuple(detached_uses)
    plain = [cuda(v) for v in operands]
    with Spy(*names) as spy:
        index_d, out_d = call(*plain)
    if fused is not None:
        assert set(fused) <= spy.used(), f"the detached call used {sorted(spy.used())}, not {sorted(fused)}"
    assert set(detached_uses) <= {n for n, _, _ in spy.calls}, f"the detached call did not use {detached_uses}"
    assert not out_d.requires_grad
    same(out_d, ref_out, "detached forward against the reference")
    if ref_index is not None:
        same(index_d, ref_index, "detached index against the reference")

    leaves = [leaf_of(v) if t else v for v, t in zip(plain, track)]
    before = [None if v is None else (v._version, v.detach().clone()) for v in leaves]
    with torch.no_grad(), Spy(*names) as spy:
        _, out_n = call(*leaves)
    if fused is not None:
        assert set(fused) <= spy.used(), f"under no_grad the call used {sorted(spy.used())}, not {sorted(fused)}"
    assert set(detached_uses) <= {n for n, _, _ in spy.calls}, f"under no_grad the call did not use {detached_uses}"
    assert out_n.grad_fn is None  # nothing recorded (a shortcut or a torch slice may hand back the input or a view of it)
    same(out_n, out_d, "no_grad forward against the detached one")

    with Spy(*names) as spy:
        index_t, out_t = call(*leaves)
    assert not (spy.used() & set(FUSED)), f"the tracked call went through {sorted(spy.used() & set(FUSED))}"
    hit = {n for n, _, _ in spy.calls} & set(forbid)
    assert not hit, f"the tracked call went through {sorted(hit)}"
    assert out_t.requires_grad, "the result of a tracked value does not require grad"
    assert out_t.grad_fn is not None or any(out_t is v for v in leaves), "the result has no grad_fn"
    same(out_t, out_d, "tracked forward against the fused one")
    if index_d is not None:
        same(index_t, index_d, "tracked index against the fused one")

    out_t.backward(cuda(coef).to(out_t.dtype))
    for i, (v, t, want) in enumerate(zip(leaves, track, ref_grads)):
        if t:
            assert v.grad is not None, f"operand {i} got no gradient"
            same(v.grad, want, f"gradient of operand {i}")
    for v, b in zip(leaves, before):
        if v is not None:
            assert v._version == b[0], "the input was written in place"
            assert torch.equal(v.detach(), b[1]), "the input changed"


# ---------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------

def distinct_keys(count, space, seed):
    """`count` distinct keys below `space`, ascending."""
    if space <= (1 << 22):
        return torch.sort(torch.randperm(space, generator=gen(seed))[:count]).values
    k = torch.unique(torch.randint(0, space, (2 * count + 64,), generator=gen(seed)))
    assert k.numel() >= count
    return torch.sort(k[torch.randperm(k.numel(), generator=gen(seed + 1))[:count]]).values


def run_lengths(size):
    if size == "edges":
        return np.array(RUNS, np.int64)
    if size == "nodups":
        return np.ones(300, np.int64)
    rng = np.random.default_rng(size)
    deg = rng.integers(1, 5, size)  # short runs, cut to `size` entries in all
    deg = deg[np.cumsum(deg) <= size]
    return np.append(deg, size - deg.sum()) if deg.sum() < size else deg


@functools.lru_cache(maxsize=None)
def coo_with_duplicates(size, m=BIG, n=BIG):
    """(index int64[2, nnz] in row-major order with equal keys adjacent, inverse, number of distinct keys)."""
    lengths = torch.as_tensor(run_lengths(size))
    lengths = lengths[lengths > 0]
    keys = distinct_keys(lengths.numel(), m * n, seed=11)
    group = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    key = keys[group]
    return torch.stack([key // n, key % n]), group, lengths.numel()


@functools.lru_cache(maxsize=None)
def csr_matrix(pow2=False, transposed=False, ncols=6001):
    """Coalesced (index, m, n): row degrees RUNS (rounded down to powers of two with pow2), distinct sorted columns
    in [1, ncols - 7): empty rows in between, column 0 and the last seven columns empty.  transposed: the same matrix
    with rows and columns swapped, in its own row-major order — long COLUMNS."""
    deg = pow2_degrees(RUNS) if pow2 else np.array(RUNS, np.int64)
    rows, cols = [], []
    for r, d in enumerate(deg):
        c = torch.sort(torch.randperm(ncols - 8, generator=gen(100 + r))[:int(d)]).values + 1
        rows.append(torch.full((int(d),), r, dtype=torch.int64))
        cols.append(c)
    index = torch.stack([torch.cat(rows), torch.cat(cols)])
    m, n = len(deg), ncols
    if transposed:
        order = torch.argsort(index[1] * m + index[0])
        index, m, n = torch.stack([index[1][order], index[0][order]]), n, m
    return index, m, n


def tensor_of(index, m, n):
    from paddle_sparse_amd import SparseTensor

    row, col = cuda(index[0].contiguous()), cuda(index[1].contiguous())
    return lambda v: SparseTensor(row=row, col=col, value=v, sparse_sizes=(m, n), is_sorted=True, trust_data=True)


def index_of(st):
    return torch.stack([st.storage.row(), st.storage.col()])


def to_csc(index, m):
    """csr2csc of a coalesced row-major index."""
    return torch.argsort(index[1] * m + index[0])


# ---------------------------------------------------------------------------------------------
# construction and coalesce
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["tensor", "storage"])
@pytest.mark.parametrize("kind,nnz", [(k, s) for k in range(len(KINDS)) for s in (1, 300)]
                         + [(0, 70_000), (1, 70_000), (3, 70_000)])
def test_unsorted_construction(kind, nnz, what):
    """SparseTensor(row, col, value) / SparseStorage(...) of unsorted entries (storage.py, the ctor's sort): a 4-byte
    scalar rides ops.sort_pairs, a tracked one goes through index_sort + gather_rows.  70 000 entries of a
    2^20 x 2^20 matrix: past the one-workgroup sort, several radix passes over 40-bit keys."""
    from paddle_sparse_amd import SparseStorage, SparseTensor

    dtype, tail = KINDS[kind]
    key = distinct_keys(nnz, BIG * BIG, seed=3)[torch.randperm(nnz, generator=gen(4))]
    row, col = cuda(key // BIG), cuda(key % BIG)
    value = gr.values(nnz, dtype, tail, seed=5)
    gr.check_values(value, gr.VALUE_MAX)
    order = torch.argsort(key)
    coef = gr.coefs((nnz,) + tail, seed=6)
    ref_out, ref_grads = gr.select_ref(value, order, coef)

    def call(v):
        if what == "tensor":
            st = SparseTensor(row=row, col=col, value=v, sparse_sizes=(BIG, BIG)).storage
        else:
            st = SparseStorage(row=row, col=col, value=v, sparse_sizes=(BIG, BIG))
        return torch.stack([st.row(), st.col()]), st.value()

    fused = {"sort_pairs"} if scalar4(dtype, tail) and nnz > 1 else None
    site(call, [value], ref_out, ref_grads, coef, fused=fused, ref_index=torch.stack([key[order] // BIG, key[order] % BIG]))


def _coalesce_case(size, layout, dtype, tail, seed=7):
    index, group, ngroups = coo_with_duplicates(size)
    nnz = index.shape[1]
    value = gr.values(nnz, dtype, tail, seed)
    gr.check_values(value, gr.VALUE_MAX)
    gr.check_sums(value.double(), group, ngroups, dtype)
    if layout == "unsorted":
        p = torch.randperm(nnz, generator=gen(seed + 1))
        index, value, group = index[:, p], value[p], group[p]
    return index, value, group, ngroups


@pytest.mark.parametrize("op", ["add", "mean"])
@pytest.mark.parametrize("kind,size,layout", [(k, "edges", lay) for k in range(len(KINDS)) for lay in ("unsorted", "sorted")]
                         + [(0, "nodups", "sorted"), (3, "nodups", "sorted"), (0, 1, "sorted"), (0, 300, "unsorted"),
                            (0, 10_241, "unsorted"), (0, 70_000, "unsorted"), (3, 70_000, "unsorted"),
                            (1, 70_000, "unsorted")])
def test_functional_coalesce(kind, size, layout, op):
    """coalesce(index, value, m, n, op) on a 2^20 x 2^20 matrix.  Detached values take ops.coalesce_chain; tracked ones
    make_keys_checked, index_sort, unique_sorted and segment_csr(perm) / gather_rows.  `nodups` sorted: the shortcut
    that returns the input keeps the graph (the result IS the tracked input)."""
    import paddle_sparse_amd as ps

    dtype, tail = KINDS[kind]
    index, value, group, ngroups = _coalesce_case(size, layout, dtype, tail)
    coef = gr.coefs((ngroups,) + tail, seed=9)
    ref_index, ref_out, ref_grads = gr.coalesce_grad_ref(index, value, BIG, BIG, op, coef)
    assert ref_index.shape[1] == ngroups
    same(ref_out, coalesce_ref(index, value, BIG, BIG, op)[1], "the two references")
    index_d = cuda(index)
    site(lambda v: ps.coalesce(index_d, v, BIG, BIG, op), [value], ref_out, ref_grads, coef, fused={"coalesce_chain"},
         ref_index=ref_index)


@pytest.mark.parametrize("kind", [0, 3, 5], ids=lambda k: KIND_IDS[k])
def test_functional_transpose(kind):
    """transpose(index, value, m, n): coalesced, the chain / the tracked stream on the swapped index; not coalesced,
    the value is handed back as it is."""
    import paddle_sparse_amd as ps

    dtype, tail = KINDS[kind]
    m, n = BIG, BIG // 2
    index, group, ngroups = coo_with_duplicates("edges", m, n)
    value = gr.values(index.shape[1], dtype, tail, seed=12)
    gr.check_sums(value.double(), group, ngroups, dtype)
    p = torch.randperm(index.shape[1], generator=gen(13))
    index, value = index[:, p], value[p]
    coef = gr.coefs((ngroups,) + tail, seed=14)
    ref_index, ref_out, ref_grads = gr.coalesce_grad_ref(index.flip(0), value, n, m, "add", coef)
    index_d = cuda(index)
    site(lambda v: ps.transpose(index_d, v, m, n), [value], ref_out, ref_grads, coef, fused={"coalesce_chain"},
         ref_index=ref_index)
    coef = gr.coefs(tuple(value.shape), seed=15)
    ref_out, ref_grads = gr.select_ref(value, torch.arange(value.shape[0]), coef)
    site(lambda v: ps.transpose(index_d, v, m, n, coalesced=False), [value], ref_out, ref_grads, coef,
         ref_index=index.flip(0))


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
def test_storage_coalesce(kind, reduce):
    """SparseTensor.coalesce(reduce) of a sorted storage with duplicates (storage.py coalesce): fp32 scalars take
    ops.unique_sorted_reduce, tracked values unique_sorted + segment_csr."""
    dtype, tail = KINDS[kind]
    index, value, group, ngroups = _coalesce_case("edges", "sorted", dtype, tail, seed=16)
    coef = gr.coefs((ngroups,) + tail, seed=17)
    ref_index, ref_out, ref_grads = gr.coalesce_grad_ref(index, value, BIG, BIG, reduce, coef)
    make = tensor_of(index, BIG, BIG)

    def call(v):
        out = make(v).coalesce(reduce)
        return index_of(out), out.storage.value()

    site(call, [value], ref_out, ref_grads, coef, fused={"unique_sorted_reduce"} if scalar4(dtype, tail) else None,
         ref_index=ref_index)


# ---------------------------------------------------------------------------------------------
# CSC order
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("entry", ["csc", "t", "t_t", "set_value_csc"])
@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
def test_csc_order(kind, entry, aligned):
    """value[csr2csc] through csc(), t(), t().t() and its inverse through set_value(v, layout="csc"): ops.gather_rows
    with the inverse permutation for the backward.  Below ops.PERMUTE_PLAN_FROM entries the detached route is the same
    gather (no fused op to ask for).  misaligned: the tracked value starts 4 bytes (2 for half types) into its buffer;
    unlike a payload, it reaches psa_gather_rows without a copy that would realign it."""
    dtype, tail = KINDS[kind]
    index, m, n = csr_matrix()
    nnz = index.shape[1]
    value = gr.values(nnz, dtype, tail, seed=20)
    gr.check_values(value, gr.VALUE_MAX)  # a permutation: nothing is added up, forward or backward
    perm = to_csc(index, m)
    sel = {"csc": perm, "t": perm, "t_t": torch.arange(nnz), "set_value_csc": torch.argsort(perm)}[entry]
    coef = gr.coefs((nnz,) + tail, seed=21)
    ref_out, ref_grads = gr.select_ref(value, sel, coef)
    make = tensor_of(index, m, n)
    base = make(None)

    def call(v):
        if entry == "csc":
            return None, make(v).csc()[2]
        if entry == "t":
            out = make(v).t()
            return index_of(out), out.storage.value()
        if entry == "t_t":
            out = make(v).t().t()
            return index_of(out), out.storage.value()
        return None, base.set_value(v, layout="csc").storage.value()

    ref_index = {"t": torch.stack([index[1][perm], index[0][perm]]), "t_t": index}.get(entry)
    site(call, [value], ref_out, ref_grads, coef, ref_index=ref_index, leaf_of=plain_leaf if aligned else misaligned_leaf)


def test_value_in_csc_order_keeps_no_memo_of_a_tracked_value():
    """Twice for a tracked value: two fresh results, both in the graph, the memo untouched; detached values are still
    memoised afterwards (the same object comes back)."""
    index, m, n = csr_matrix()
    value = gr.values(index.shape[1], F32, (), seed=22)
    perm = to_csc(index, m)
    v = cuda(value).requires_grad_(True)
    st = tensor_of(index, m, n)(v).storage
    first, second = st._value_in_csc_order(), st._value_in_csc_order()
    assert first is not second and first.grad_fn is not None and second.grad_fn is not None
    assert st._value_csc_memo is None
    coef = gr.coefs(value.shape[0], seed=23)
    (first * cuda(coef).float() + second).sum().backward()
    _, (g1,) = gr.select_ref(value, perm, coef)
    _, (g2,) = gr.select_ref(value, perm, torch.ones_like(coef))
    same(v.grad, g1 + g2, "gradient through two gathers")
    plain = tensor_of(index, m, n)(cuda(value)).storage
    a, b = plain._value_in_csc_order(), plain._value_in_csc_order()
    assert a is b and not a.requires_grad
    same(a, value[perm], "memoised CSC values")
    with torch.no_grad():  # a requires_grad value outside of autograd is memoised too
        assert st._value_in_csc_order() is st._value_in_csc_order()


def test_coalesce_of_a_misaligned_tracked_value():
    """The tracked coalesce reads the value through segment_csr(perm) and gather_rows from wherever it lies."""
    import paddle_sparse_amd as ps

    for tail in ((), (3,)):
        index, value, group, ngroups = _coalesce_case("edges", "unsorted", F32, tail, seed=24)
        coef = gr.coefs((ngroups,) + tail, seed=25)
        for op in ("add", "mean"):
            ref_index, ref_out, ref_grads = gr.coalesce_grad_ref(index, value, BIG, BIG, op, coef)
            index_d = cuda(index)
            site(lambda v: ps.coalesce(index_d, v, BIG, BIG, op), [value], ref_out, ref_grads, coef,
                 fused={"coalesce_chain"}, ref_index=ref_index, leaf_of=misaligned_leaf)


# ---------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache", ["cold", "filled"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("dim", [0, 1])
@pytest.mark.parametrize("transposed", [False, True], ids=["long_rows", "long_columns"])
@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
def test_reduce_over_a_sparse_dim(kind, transposed, dim, reduce, cache):
    """sum / mean over rows (segment_csr over rowptr) and over columns.  dim=0 with DETACHED fp32 / fp64 values of a
    small cold storage scatters with atomics (ops.scatter, which autograd cannot follow); tracked values always take
    segment_csr over the CSC view, so a cold and a cached storage give the same gradient."""
    dtype, tail = KINDS[kind]
    index, m, n = csr_matrix(transposed=transposed)
    value = gr.values(index.shape[1], dtype, tail, seed=30)
    if transposed:  # values drawn in the order of the long runs, so that a half type's (v, -v) pairs stay inside them
        first = csr_matrix()[0]
        value = value[torch.argsort(first[1] * n + first[0])]
    size = (n, m)[dim]
    gr.check_sums(value.double(), index[1 - dim], size, dtype)
    coef = gr.coefs((size,) + tail, seed=31)
    gr.check_sums(coef[index[1 - dim]], torch.arange(index.shape[1]), index.shape[1], dtype)  # one term per element
    ref_out, ref_grads = gr.reduce_grad_ref(index, value, m, n, dim, reduce, coef)
    same(ref_out, group_reduce(value, index[1 - dim], size, reduce), "the two references")
    make = tensor_of(index, m, n)

    def call(v):
        a = make(v)
        if cache == "filled":
            a.fill_cache_()
        return None, getattr(a, reduce)(dim)

    scatters = dim == 0 and cache == "cold" and dtype not in HALF_TYPES
    site(call, [value], ref_out, ref_grads, coef, forbid=("scatter",), detached_uses=("scatter",) if scatters else ())


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_reduce_over_everything_and_over_value_dims(reduce):
    """dim=None and dim >= 2 are the framework's reducers on the value tensor.  Its mean multiplies by a rounded
    1 / count, so the counts here are powers of two (256 entries; value dims of 2)."""
    deg = np.array([0, 128, 64, 0, 64], np.int64)
    rows = torch.repeat_interleave(torch.arange(deg.size), torch.as_tensor(deg))
    cols = torch.cat([torch.sort(torch.randperm(300, generator=gen(r))[:int(d)]).values for r, d in enumerate(deg)])
    index = torch.stack([rows, cols])
    make = tensor_of(index, deg.size, 300)
    for dtype, tail, dims in ((F32, (), (None,)), (F64, (), (None,)), (F32, (2, 2), (None, 2, 3, -1)), (F16, (), (None,))):
        value = gr.values(256, dtype, tail, seed=32)
        for dim in dims:
            where = dim if dim is None or dim >= 0 else 2 + len(tail) + dim
            ref_shape = gr.reduce_grad_ref(index, value, deg.size, 300, where, reduce)[0].shape
            coef = gr.coefs(tuple(ref_shape), seed=33)
            ref_out, ref_grads = gr.reduce_grad_ref(index, value, deg.size, 300, where, reduce, coef)
            site(lambda v: (None, getattr(make(v), reduce)(dim)), [value], ref_out, ref_grads, coef)


def test_reduce_over_columns_at_the_sort_threshold():
    """(1 << 20) + 3 entries, one case: from storage._SORT_BEATS_ATOMICS entries detached values leave the scatter for
    the CSC segments too.  Tracked and detached then run the same reducer; min / max raise here as they do below."""
    from paddle_sparse_amd.storage import _SORT_BEATS_ATOMICS

    m, n, nnz = 2049, 1031, (1 << 20) + 3
    assert nnz >= _SORT_BEATS_ATOMICS
    key = distinct_keys(nnz, m * n, seed=40)
    index = torch.stack([key // n, key % n])
    value = gr.values(nnz, F32, (), seed=41)
    gr.check_sums(value.double(), index[1], n, F32)
    coef = gr.coefs(n, seed=42)
    make = tensor_of(index, m, n)
    for reduce in ("sum", "mean"):
        ref_out, ref_grads = gr.reduce_grad_ref(index, value, m, n, 0, reduce, coef)
        site(lambda v: (None, getattr(make(v), reduce)(0)), [value], ref_out, ref_grads, coef, forbid=("scatter",))
    v = cuda(value).requires_grad_(True)
    for reduce in ("min", "max"):
        with pytest.raises(NotImplementedError, match="not differentiable"):
            getattr(make(v), reduce)(0)
        same(getattr(make(v.detach()), reduce)(0), group_reduce(value, index[1], n, reduce), f"detached {reduce}")

    # from ops.PERMUTE_PLAN_FROM four-byte entries the SECOND request for value[csr2csc] on one structure (a new value
    # object: the next training step) goes through the planned ops.permute_apply; a tracked value on that same
    # structure, plan and all, does not
    from paddle_sparse_amd import ops

    assert nnz >= ops.PERMUTE_PLAN_FROM
    ref_out, ref_grads = gr.reduce_grad_ref(index, value, m, n, 0, "sum", coef)
    first = make(cuda(value))
    with Spy("permute_apply") as spy:
        same(first.sum(0), ref_out, "first detached request")
        assert not spy.calls, "the first request already planned the permutation"
        second = first.set_value(cuda(value).clone(), layout="coo")
        same(second.sum(0), ref_out, "second detached request")
        assert spy.calls, "the second detached request did not go through permute_apply"
    leaf = plain_leaf(cuda(value))
    with Spy("permute_apply") as spy:
        out = second.set_value(leaf, layout="coo").sum(0)
        with torch.no_grad():
            same(second.set_value(leaf, layout="coo").sum(0), ref_out, "no_grad request on the planned structure")
        assert len(spy.calls) == 1, "permute_apply serves the no_grad request, and only that one"
    same(out, ref_out, "tracked request on the planned structure")
    out.backward(cuda(coef).float())
    same(leaf.grad, ref_grads[0], "gradient on the planned structure")


# ---------------------------------------------------------------------------------------------
# sparse + sparse, sparse * sparse, to_symmetric
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def two_operands(na, nb, m=BIG, n=BIG):
    """Two coalesced indices that share about half of their entries."""
    keys = distinct_keys(na + nb - min(na, nb) // 2, m * n, seed=50)
    p = torch.randperm(keys.numel(), generator=gen(51))
    ka, kb = torch.sort(keys[p[:na]]).values, torch.sort(keys[p[-nb:]]).values
    assert min(na, nb) < 4 or 0 < np.intersect1d(ka.numpy(), kb.numpy()).size < min(na, nb)
    return torch.stack([ka // n, ka % n]), torch.stack([kb // n, kb % n])


@pytest.mark.parametrize("track", [(True, False), (False, True), (True, True)], ids=["a", "b", "both"])
@pytest.mark.parametrize("na,nb", [(1, 1), (150, 150), (5121, 5120)], ids=["2", "300", "10241"])
@pytest.mark.parametrize("kind", [0, 1, 3, 5, 6], ids=lambda k: KIND_IDS[k])
def test_sparse_add(kind, na, nb, track):
    """A + B: up to coalesce._ONE_WORKGROUP_BELOW (10 240) entries in all through the coalesce of the concatenation
    (detached: ops.coalesce_chain), above through the merge of the two sorted streams (detached fp32 scalars:
    ops.merge_sorted with payloads + ops.unique_sorted_reduce)."""
    from paddle_sparse_amd.coalesce import _ONE_WORKGROUP_BELOW

    dtype, tail = KINDS[kind]
    index_a, index_b = two_operands(na, nb)
    va, vb = gr.values(na, dtype, tail, seed=52), gr.values(nb, dtype, tail, seed=53)
    gr.check_values(va, gr.VALUE_MAX), gr.check_values(vb, gr.VALUE_MAX)
    both = torch.cat([index_a[0] * BIG + index_a[1], index_b[0] * BIG + index_b[1]])
    gr.check_sums(torch.cat([va, vb]).double(), torch.unique(both, return_inverse=True)[1], both.numel(), dtype)
    above = na + nb > _ONE_WORKGROUP_BELOW
    assert above == (na + nb == 10_241)
    make_a, make_b = tensor_of(index_a, BIG, BIG), tensor_of(index_b, BIG, BIG)
    ref_index = gr.add_grad_ref(index_a, va, index_b, vb, BIG, BIG)[0]
    coef = gr.coefs((ref_index.shape[1],) + tail, seed=54)
    ref_index, ref_out, ref_grads = gr.add_grad_ref(index_a, va, index_b, vb, BIG, BIG, coef)

    def call(a, b):
        out = make_a(a) + make_b(b)
        return index_of(out), out.storage.value()

    fused = ({"merge_sorted", "unique_sorted_reduce"} if scalar4(dtype, tail) else None) if above else {"coalesce_chain"}
    site(call, [va, vb], ref_out, ref_grads, coef, fused=fused, track=track, ref_index=ref_index)


@pytest.mark.parametrize("na,nb", [(150, 150), (5121, 5120)], ids=["300", "10241"])
def test_sparse_add_with_a_value_less_operand(na, nb):
    """The sum has values only when both operands do (add.py): a tracked value beside a value-less operand changes
    neither the entries nor that rule."""
    index_a, index_b = two_operands(na, nb)
    ref_index = gr.add_grad_ref(index_a, gr.values(na, F32), index_b, gr.values(nb, F32), BIG, BIG)[0]
    v = cuda(gr.values(na, F32, (), seed=55)).requires_grad_(True)
    for out in (tensor_of(index_a, BIG, BIG)(v) + tensor_of(index_b, BIG, BIG)(None),
                tensor_of(index_b, BIG, BIG)(None) + tensor_of(index_a, BIG, BIG)(v)):
        assert out.storage.value() is None
        same(index_of(out), ref_index, "entries of the sum")
    assert v._version == 0


@pytest.mark.parametrize("track", [(True, False), (False, True), (True, True)], ids=["a", "b", "both"])
@pytest.mark.parametrize("kind", [0, 1, 3, 5, 6], ids=lambda k: KIND_IDS[k])
def test_sparse_mul(kind, track):
    """A * B with partial overlap: detached fp32 scalars ride ops.merge_sorted, tracked ones are gathered through the
    merge's source array; the gradient of each operand is the other's value on the shared entries, 0 elsewhere."""
    dtype, tail = KINDS[kind]
    index_a, index_b = two_operands(5121, 5120)
    va, vb = gr.values(5121, dtype, tail, seed=56), gr.values(5120, dtype, tail, seed=57)
    gr.check_values(va, gr.VALUE_MAX), gr.check_values(vb, gr.VALUE_MAX)  # one product per entry: nothing is added up
    make_a, make_b = tensor_of(index_a, BIG, BIG), tensor_of(index_b, BIG, BIG)
    ref_index = gr.mul_grad_ref(index_a, va, index_b, vb, BIG, BIG)[0]
    coef = gr.coefs((ref_index.shape[1],) + tail, seed=58)
    ref_index, ref_out, ref_grads = gr.mul_grad_ref(index_a, va, index_b, vb, BIG, BIG, coef)

    def call(a, b):
        out = make_a(a) * make_b(b)
        return index_of(out), out.storage.value()

    site(call, [va, vb], ref_out, ref_grads, coef, fused={"merge_sorted"} if scalar4(dtype, tail) else None, track=track,
         ref_index=ref_index)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("kind,nnz", [(k, 3000) for k in (0, 1, 3, 5, 6)] + [(0, 33_000), (3, 33_000)])
def test_to_symmetric(kind, nnz, reduce):
    """Up to tensor._MERGE_ABOVE (65 536) keys one sort of [A; A^T] and segment_csr(perm) (both routes alike); above,
    the merge of A with its CSC view (detached fp32 scalars: ops.merge_sorted with payloads).  Diagonal entries and
    mirrored pairs meet themselves: runs of two, so the mean's quotients add up exactly."""
    from paddle_sparse_amd.tensor import _MERGE_ABOVE

    dtype, tail = KINDS[kind]
    N = 1 << 16
    key = distinct_keys(nnz, N * N, seed=60)
    r, c = key // N, key % N
    extra = torch.cat([c[:200] * N + r[:200], r[200:300] * N + r[200:300]])  # mirrors and diagonal entries
    key = torch.unique(torch.cat([key, extra]))
    index = torch.stack([key // N, key % N])
    value = gr.values(key.numel(), dtype, tail, seed=61)
    gr.check_values(value, gr.VALUE_MAX)
    laid = torch.cat([index[0] * N + index[1], index[1] * N + index[0]])
    gr.check_sums(torch.cat([value, value]).double(), torch.unique(laid, return_inverse=True)[1], laid.numel(), dtype)
    ref_index = gr.symmetric_grad_ref(index, value, N, reduce)[0]
    assert ref_index.shape[1] < 2 * key.numel()
    coef = gr.coefs((ref_index.shape[1],) + tail, seed=62)
    ref_index, ref_out, ref_grads = gr.symmetric_grad_ref(index, value, N, reduce, coef)
    make = tensor_of(index, N, N)

    def call(v):
        out = make(v).to_symmetric(reduce)
        assert out.sparse_sizes() == (N, N)
        return index_of(out), out.storage.value()

    above = 2 * key.numel() > _MERGE_ABOVE
    assert above == (nnz == 33_000)
    site(call, [value], ref_out, ref_grads, coef, fused={"merge_sorted"} if above and scalar4(dtype, tail) else None,
         ref_index=ref_index)


# ---------------------------------------------------------------------------------------------
# dense broadcast and selections
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["column", "row"])
@pytest.mark.parametrize("kind_op", ["add", "mul"])
@pytest.mark.parametrize("dtype", [F32, F64, F16, BF16], ids=str)
@pytest.mark.parametrize("transposed", [False, True], ids=["long_rows", "long_columns"])
def test_dense_broadcast(transposed, dtype, kind_op, shape):
    """A + w / A * w for w of shape (M, 1) or (1, N) that requires grad: the gradient of w is the scatter-add of
    _GatherRows.backward over row / col, that of the value is the coefficient (times the spread operand)."""
    index, m, n = csr_matrix(transposed=transposed)
    nnz = index.shape[1]
    value = gr.values(nnz, dtype, (), seed=70)
    vec = gr.integers((m, 1) if shape == "column" else (1, n), -gr.COEF_MAX, gr.COEF_MAX, dtype, seed=71)
    gr.check_values(value, gr.VALUE_MAX), gr.check_values(vec, gr.COEF_MAX)
    coef = gr.coefs(nnz, seed=72)
    if dtype in HALF_TYPES:  # the gradient of w has to be an integer the type holds: (c, -c) pairs along the long runs
        order = torch.argsort(index[0] * n + index[1]) if shape == "column" else torch.argsort(index[1] * m + index[0])
        c = coef[order]
        c[1::2] = -c[0:nnz - (nnz % 2):2]
        if kind_op == "mul":  # the terms are coef * value: equal values within a pair
            v = value[order]
            v[1::2] = v[0:nnz - (nnz % 2):2]
            value[order] = v
        coef[order] = c + 0.0
    which = index[0] if shape == "column" else index[1]
    terms = coef * (value.double() if kind_op == "mul" else 1.0)
    gr.check_sums(terms, which, vec.numel(), dtype)  # what the scatter-add into grad_w adds up
    ref_out, ref_grads = gr.broadcast_grad_ref(index, value, vec, kind_op, coef)
    make = tensor_of(index, m, n)
    site(lambda v, w: (None, getattr(make(v), kind_op)(w).storage.value()), [value, vec], ref_out, ref_grads, coef)
    for track in ((True, False), (False, True)):
        site(lambda v, w: (None, getattr(make(v), kind_op)(w).storage.value()), [value, vec], ref_out, ref_grads, coef,
             track=track)


def _selection(entry, index, m, n):
    """(positions of the selected entries in storage order, index of the result, the call)."""
    row, col = index
    nnz = row.numel()
    rowptr = torch.zeros(m + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=m), 0)
    long_row = int(torch.bincount(row, minlength=m).argmax())
    if entry in ("rows", "row_mask"):
        if entry == "rows":  # repeats, empty rows, the long row
            idx = torch.tensor([long_row, long_row, 0, 4, long_row, 3, 9, 9, m - 1])
            call = lambda a: a.index_select(0, cuda(idx))
        else:
            mask = torch.rand(m, generator=gen(80)) < 0.6
            idx = mask.nonzero().view(-1)
            call = lambda a: a.masked_select(0, cuda(mask))
        sel = torch.cat([torch.arange(int(rowptr[i]), int(rowptr[i + 1])) for i in idx])
        new_row = torch.repeat_interleave(torch.arange(idx.numel()), rowptr[idx + 1] - rowptr[idx])
        return sel, torch.stack([new_row, col[sel]]), call
    if entry in ("cols", "col_mask"):
        if entry == "cols":
            busy = int(torch.bincount(col, minlength=n).argmax())
            idx = torch.tensor([busy, 0, busy, 17, n - 1, 18, 18, busy])
            call = lambda a: a.index_select(1, cuda(idx))
        else:
            mask = torch.rand(n, generator=gen(81)) < 0.5
            idx = mask.nonzero().view(-1)
            call = lambda a: a.masked_select(1, cuda(mask))
        picks = [(col == j).nonzero().view(-1) for j in idx.tolist()]
        sel = torch.cat(picks)
        new_col = torch.repeat_interleave(torch.arange(idx.numel()), torch.tensor([p.numel() for p in picks]))
        order = torch.argsort(row[sel] * idx.numel() + new_col)
        sel = sel[order]
        return sel, torch.stack([row[sel], new_col[order]]), call
    if entry == "nnz":
        idx = torch.sort(torch.randint(0, nnz, (nnz // 3,), generator=gen(82))).values  # ascending, with repeats
        return idx, index[:, idx], lambda a: a.index_select_nnz(cuda(idx), layout="coo")
    if entry == "narrow_rows":
        start, length = 3, 13
        sel = torch.arange(int(rowptr[start]), int(rowptr[start + length]))
        return sel, torch.stack([row[sel] - start, col[sel]]), lambda a: a.narrow(0, start, length)
    start, length = n // 3, n // 2  # narrow_cols
    sel = ((col >= start) & (col < start + length)).nonzero().view(-1)
    return sel, torch.stack([row[sel], col[sel] - start]), lambda a: a.narrow(1, start, length)


@pytest.mark.parametrize("entry", ["rows", "row_mask", "cols", "col_mask", "nnz", "narrow_rows", "narrow_cols"])
@pytest.mark.parametrize("kind", range(len(KINDS)), ids=KIND_IDS)
def test_selections(kind, entry):
    """index_select(0 / 1) with repeats and empty rows / columns, masked_select, index_select_nnz, narrow: gathers (and
    torch slices for narrow); a repeated entry collects the gradient of every copy."""
    dtype, tail = KINDS[kind]
    index, m, n = csr_matrix()
    value = gr.values(index.shape[1], dtype, tail, seed=83)
    sel, ref_index, select = _selection(entry, index, m, n)
    coef = gr.coefs((sel.numel(),) + tail, seed=84)
    gr.check_sums(coef, sel, index.shape[1], dtype)  # what a repeated entry collects
    ref_out, ref_grads = gr.select_ref(value, sel, coef)
    make = tensor_of(index, m, n)

    def call(v):
        out = select(make(v))
        return index_of(out), out.storage.value()

    site(call, [value], ref_out, ref_grads, coef, ref_index=ref_index)


@pytest.mark.parametrize("dtype", [F32, F64, BF16], ids=str)
def test_mean_after_a_repeated_selection(dtype):
    """index_select(0, rows with repeats).mean(dim=1): several quotients coef / degree land on one entry.  Row degrees
    are powers of two (exact_ref.pow2_degrees), so their sum is exact."""
    index, m, n = csr_matrix(pow2=True)
    deg = torch.bincount(index[0], minlength=m)
    gr.check_pow2(deg)
    rowptr = torch.zeros(m + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    idx = torch.tensor([15, 15, 0, 4, 15, 5, 9, 9, 13, 13, 13, 13])
    sel = torch.cat([torch.arange(int(rowptr[i]), int(rowptr[i + 1])) for i in idx])
    group = torch.repeat_interleave(torch.arange(idx.numel()), deg[idx])
    value = gr.values(index.shape[1], dtype, (), seed=85)
    gr.check_sums(value.double()[sel], group, idx.numel(), dtype)
    coef = gr.coefs(idx.numel(), seed=86)
    scale = float(deg.max())  # every term coef / 2^j is a multiple of 1 / scale
    gr.check_sums((coef[group] / deg[idx][group].double()) * scale, sel, index.shape[1], F32)
    make = tensor_of(index, m, n)
    for reduce in ("sum", "mean"):
        ref_out, ref_grads = gr.select_reduce_grad_ref(value, sel, group, idx.numel(), reduce, coef)
        site(lambda v: (None, getattr(make(v).index_select(0, cuda(idx)), reduce)(1)), [value], ref_out, ref_grads, coef)


# ---------------------------------------------------------------------------------------------
# spspmm
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def product_operands(nnz):
    m, k, n = 300, 200, 250
    ka, kb = distinct_keys(nnz, m * k, seed=90), distinct_keys(nnz, k * n, seed=91)
    return torch.stack([ka // k, ka % k]), torch.stack([kb // n, kb % n]), m, k, n


@pytest.mark.parametrize("entry", ["spspmm", "matmul"])
@pytest.mark.parametrize("track", [(True, False), (False, True), (True, True)], ids=["a", "b", "both"])
@pytest.mark.parametrize("dtype,nnz", [(F32, 1), (F32, 300), (F32, 6000), (F64, 300), (F64, 6000)])
def test_spspmm(dtype, nnz, track, entry):
    """spspmm(...) and A @ B for sparse B, gradient wrt valueA, valueB and both: detached fp32 values walk the CSC
    views and ride ops.sort_pairs_field; tracked values take gather_rows of both operands per partial product, their
    product, index_sort and segment_csr(perm)."""
    import paddle_sparse_amd as ps

    index_a, index_b, m, k, n = product_operands(nnz)
    va, vb = gr.values(nnz, dtype, (), seed=92), gr.values(nnz, dtype, (), seed=93)
    key, prod = spspmm_terms(index_a, va, index_b, vb, m, k, n)
    if key.numel():
        gr.check_sums(prod, torch.unique(key, return_inverse=True)[1], int(key.numel()), dtype)
    longest = max(int(torch.bincount(index_b[0], minlength=k).max()), int(torch.bincount(index_a[1], minlength=k).max()))
    assert longest * gr.VALUE_MAX * gr.COEF_MAX < (1 << 24)  # the sums of either gradient
    ref_index = gr.spspmm_grad_ref(index_a, va, index_b, vb, m, k, n)[0]
    coef = gr.coefs(ref_index.shape[1], seed=94)
    ref_index, ref_out, ref_grads = gr.spspmm_grad_ref(index_a, va, index_b, vb, m, k, n, coef)
    ia, ib = cuda(index_a), cuda(index_b)
    make_a, make_b = tensor_of(index_a, m, k), tensor_of(index_b, k, n)

    def call(a, b):
        if entry == "spspmm":
            return ps.spspmm(ia, a, ib, b, m, k, n)
        out = make_a(a) @ make_b(b)
        return index_of(out), out.storage.value()

    fused = {"sort_pairs_field", "unique_sorted_reduce"} if dtype == F32 and ref_index.shape[1] > 0 else None
    site(call, [va, vb], ref_out, ref_grads, coef, fused=fused, track=track, ref_index=ref_index)


@pytest.mark.parametrize("entry", ["spspmm", "matmul"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_spspmm_with_a_value_less_operand(dtype, entry):
    """An operand without values counts as ones and the other one still gets its gradient."""
    import paddle_sparse_amd as ps

    index_a, index_b, m, k, n = product_operands(300)
    v = gr.values(300, dtype, (), seed=95)
    ia, ib = cuda(index_a), cuda(index_b)
    make_a, make_b = tensor_of(index_a, m, k), tensor_of(index_b, k, n)
    fused = {"sort_pairs_field", "unique_sorted_reduce"} if dtype == F32 else None
    for side in (0, 1):
        operands = [v, None] if side == 0 else [None, v]
        ref_index = gr.spspmm_grad_ref(index_a, operands[0], index_b, operands[1], m, k, n)[0]
        coef = gr.coefs(ref_index.shape[1], seed=96)
        ref_index, ref_out, ref_grads = gr.spspmm_grad_ref(index_a, operands[0], index_b, operands[1], m, k, n, coef)

        def call(x):
            a, b = (x, None) if side == 0 else (None, x)
            if entry == "spspmm":
                return ps.spspmm(ia, a, ib, b, m, k, n)
            out = make_a(a) @ make_b(b)
            return index_of(out), out.storage.value()

        site(call, [v], ref_out, [ref_grads[side]], coef, fused=fused, ref_index=ref_index)


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
@pytest.mark.parametrize("short", ["a", "b"])
def test_spspmm_refuses_values_of_the_wrong_length_tracked_or_not(short, dtype):
    """A value array shorter than its index is refused on both routes (detached: the storage's assertion for fp32,
    spspmm_expand's ValueError for fp64); on the tracked one with that ValueError and before anything is launched
    (ops.gather_rows would read past the array): no op of `ops` has been called when it raises."""
    import paddle_sparse_amd as ps

    index_a, index_b, m, k, n = product_operands(300)
    va = cuda(gr.values(300 if short == "b" else 299, dtype, (), seed=97))
    vb = cuda(gr.values(300 if short == "a" else 299, dtype, (), seed=98))
    with pytest.raises(AssertionError if dtype == F32 else ValueError):
        ps.spspmm(cuda(index_a), va, cuda(index_b), vb, m, k, n)
    launches = ("ind2ptr", "spspmm_count", "count2ptr", "ptr2ind", "spspmm_expand", "gather_rows", "index_sort")
    for track in ((True, False), (False, True), (True, True)):
        a, b = (x.clone().requires_grad_(t) for x, t in zip((va, vb), track))
        with Spy(*launches) as spy, pytest.raises(ValueError, match="one entry per index"):
            ps.spspmm(cuda(index_a), a, cuda(index_b), b, m, k, n)
        assert not spy.calls, f"launched {[c[0] for c in spy.calls]} before raising"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=str)
def test_spspmm_refuses_half_values_tracked_or_not(dtype):
    """The product has no half-precision kernel: TypeError, for a tracked value as for a detached one."""
    import paddle_sparse_amd as ps

    index_a, index_b, m, k, n = product_operands(300)
    va, vb = cuda(gr.values(300, dtype, (), seed=97)), cuda(gr.values(300, dtype, (), seed=98))
    for a in (va, va.clone().requires_grad_(True)):
        with pytest.raises(TypeError):
            ps.spspmm(cuda(index_a), a, cuda(index_b), vb, m, k, n)
        with pytest.raises(TypeError):
            tensor_of(index_a, m, k)(a) @ tensor_of(index_b, k, n)(vb)


# ---------------------------------------------------------------------------------------------
# min / max, empty inputs
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduce", ["min", "max"])
def test_min_max_of_tracked_values_raise_everywhere(reduce):
    """min / max are not differentiable in this build: every entry point that reduces tracked values with them raises
    the NotImplementedError of _SegmentCsr — also dim=0 of a small cold storage, where detached values scatter — and
    the detached result is unchanged."""
    import paddle_sparse_amd as ps

    msg = "not differentiable"
    index, value, group, ngroups = _coalesce_case("edges", "unsorted", F32, ())
    v = cuda(value).requires_grad_(True)
    with pytest.raises(NotImplementedError, match=msg):
        ps.coalesce(cuda(index), v, BIG, BIG, reduce)
    same(ps.coalesce(cuda(index), v.detach(), BIG, BIG, reduce)[1], coalesce_ref(index, value, BIG, BIG, reduce)[1],
         "detached coalesce")
    index, value, group, ngroups = _coalesce_case("edges", "sorted", F32, ())
    v = cuda(value).requires_grad_(True)
    with pytest.raises(NotImplementedError, match=msg):
        tensor_of(index, BIG, BIG)(v).coalesce(reduce)
    same(tensor_of(index, BIG, BIG)(v.detach()).coalesce(reduce).storage.value(),
         coalesce_ref(index, value, BIG, BIG, reduce)[1], "detached storage coalesce")

    for dtype in (F32, F64, F16):
        index, m, n = csr_matrix()
        value = gr.values(index.shape[1], dtype, (), seed=99)
        v = cuda(value).requires_grad_(True)
        make = tensor_of(index, m, n)
        for dim in (0, 1):
            for filled in (False, True):
                a = make(v)
                if filled:
                    a.fill_cache_()
                with pytest.raises(NotImplementedError, match=msg):
                    getattr(a, reduce)(dim)
                with torch.no_grad():
                    same(getattr(make(v), reduce)(dim), group_reduce(value, index[1 - dim], (n, m)[dim], reduce),
                         f"{reduce} over dim {dim} without autograd")

    # dim=None and value dims are the framework's reducers: differentiable, the gradient goes to the extreme
    index, m, n = csr_matrix()
    value = torch.arange(index.shape[1] * 2, dtype=F32).view(-1, 2)  # no ties
    v = cuda(value).requires_grad_(True)
    getattr(tensor_of(index, m, n)(v), reduce)().backward()
    where = int(value.argmin() if reduce == "min" else value.argmax())
    assert v.grad.view(-1)[where] == 1 and float(v.grad.abs().sum()) == 1
    v.grad = None
    out = getattr(tensor_of(index, m, n)(v), reduce)(2)
    same(out, value.amin(1) if reduce == "min" else value.amax(1), f"{reduce} over a value dim")
    out.sum().backward()
    want = torch.zeros_like(value)
    want[:, 0 if reduce == "min" else 1] = 1
    same(v.grad, want, f"gradient of {reduce} over a value dim")

    N = 1 << 16
    for nnz in (3000, 33_000):  # below and above tensor._MERGE_ABOVE keys
        key = distinct_keys(nnz, N * N, seed=60)
        key = torch.unique(torch.cat([key, (key[:200] % N) * N + key[:200] // N]))
        index = torch.stack([key // N, key % N])
        v = cuda(gr.values(key.numel(), F32, (), seed=61)).requires_grad_(True)
        with pytest.raises(NotImplementedError, match=msg):
            tensor_of(index, N, N)(v).to_symmetric(reduce)
        assert not tensor_of(index, N, N)(v.detach()).to_symmetric(reduce).storage.value().requires_grad


@pytest.mark.parametrize("dtype", [F32, F64, F16], ids=str)
def test_nothing_stored(dtype):
    """nnz 0: every site hands back an empty result that is still part of the graph, and backward gives an empty
    gradient."""
    import paddle_sparse_amd as ps
    from paddle_sparse_amd import SparseTensor

    empty_i = torch.empty(0, dtype=torch.int64).cuda()

    def leaf():
        return torch.empty(0, dtype=dtype).cuda().requires_grad_(True)

    def check(out, v, shape):
        assert tuple(out.shape) == shape and out.requires_grad
        out.sum().backward()
        assert v.grad is not None and v.grad.shape == v.shape

    v = leaf()
    a = SparseTensor(row=empty_i, col=empty_i, value=v, sparse_sizes=(5, 7))
    check(a.storage.value(), v, (0,))
    v = leaf()
    check(ps.coalesce(torch.stack([empty_i, empty_i]), v, 5, 7)[1], v, (0,))
    for call, shape in ((lambda a: a.csc()[2], (0,)), (lambda a: a.t().storage.value(), (0,)),
                        (lambda a: a.coalesce("mean").storage.value(), (0,)), (lambda a: a.sum(1), (5,)),
                        (lambda a: a.mean(0), (7,)), (lambda a: a.sum(0), (7,)),
                        (lambda a: a.index_select(0, torch.tensor([1, 1]).cuda()).storage.value(), (0,)),
                        (lambda a: a.index_select(1, torch.tensor([1, 1]).cuda()).storage.value(), (0,))):
        v = leaf()
        out = call(SparseTensor(row=empty_i, col=empty_i, value=v, sparse_sizes=(5, 7), is_sorted=True))
        check(out, v, shape)
        assert float(out.detach().abs().sum()) == 0.0

    def empty(v):
        return SparseTensor(row=empty_i, col=empty_i, value=v, sparse_sizes=(6, 6), is_sorted=True)

    w = torch.ones(2, dtype=dtype).cuda()
    full = SparseTensor(row=torch.tensor([0, 3]).cuda(), col=torch.tensor([1, 5]).cuda(), value=w, sparse_sizes=(6, 6),
                        is_sorted=True)
    two_sided = [(lambda a, b: (a + b).storage.value(), 0), (lambda a, b: (a * b).storage.value(), 0)]
    if dtype != F16:  # the product takes fp32 / fp64 (test_spspmm_refuses_half_values_tracked_or_not)
        two_sided += [(lambda a, b: (a @ b).storage.value(), 0),
                      (lambda a, b: ps.spspmm(index_of(a), a.storage.value(), index_of(b), b.storage.value(), 6, 6, 6)[1], 0)]
    for call, _ in two_sided:
        va, vb = leaf(), leaf()
        out = call(empty(va), empty(vb))  # both empty and tracked
        assert tuple(out.shape) == (0,) and out.requires_grad
        out.sum().backward()
        assert va.grad.shape == (0,) and vb.grad.shape == (0,)
        for swap in (False, True):  # an empty tracked operand beside a stored, detached one
            v = leaf()
            out = call(full, empty(v)) if swap else call(empty(v), full)
            assert out.requires_grad and out.dtype == dtype
            out.sum().backward()
            assert v.grad is not None and v.grad.shape == (0,)
    v = leaf()
    sym = empty(v).to_symmetric("mean")
    check(sym.storage.value(), v, (0,))
    assert sym.sparse_sizes() == (6, 6)
