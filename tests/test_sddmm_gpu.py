"""GPU suite of sddmm and of the attention step softmax(sddmm(A, q, k)) @ v.

Exact throughout: with small integers in the dense operands every dot and every gradient is an
exactly representable integer (or, behind a softmax over power-of-two degrees with equal scores, a
dyadic rational), so the results equal dense float64 autograd of ((x @ y.T) * mask) bit for bit."""
import numpy as np
import pytest
import torch

import softmax_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 4099, 70001]


def pattern(rng, lens, N):
    """Sorted CSR pattern with the given row lengths, distinct columns inside a row."""
    cols = [np.sort(rng.choice(N, size=ln, replace=False)) for ln in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rowptr, np.concatenate(cols).astype(np.int64)


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def dense_reference(rowptr, col, x, y, g):
    """float64 autograd of ((x @ y.T) * W).sum() with W the entry weights g added up per cell."""
    M, N = rowptr.size - 1, y.shape[0]
    row = np.repeat(np.arange(M), np.diff(rowptr))
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    yt = torch.from_numpy(y.astype(np.float64)).requires_grad_()
    W = torch.zeros(M, N, dtype=torch.float64)
    W.index_put_((torch.from_numpy(row), torch.from_numpy(col)), torch.from_numpy(g.astype(np.float64)), accumulate=True)
    scores = xt @ yt.T
    (scores * W).sum().backward()
    return scores.detach().numpy()[row, col], xt.grad.numpy(), yt.grad.numpy()


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(41)
    N = 70001
    rowptr, col = pattern(rng, LENGTHS, N)
    return rowptr, col, N


@pytest.mark.parametrize("K", [1, 3, 4, 64, 65, 128, 200])
def test_sddmm_exact_forward_and_gradients(big, K):
    import paddle_sparse_amd as psa

    rowptr, col, N = big
    M = rowptr.size - 1
    rng = np.random.default_rng(50 + K)
    x, y = ints(rng, (M, K), -4, 4), ints(rng, (N, K), -4, 4)
    g = ints(rng, col.size, -2, 2)
    want, want_gx, want_gy = dense_reference(rowptr, col, x, y, g)
    A = psa.SparseTensor(rowptr=torch.from_numpy(rowptr).to(DEV), col=torch.from_numpy(col).to(DEV),
                         sparse_sizes=(M, N), is_sorted=True)
    xd = torch.from_numpy(x).to(DEV).requires_grad_()
    yd = torch.from_numpy(y).to(DEV).requires_grad_()
    out = psa.sddmm(A, xd, yd)
    v = out.storage.value()
    assert v.dtype == torch.float32 and v.shape == (col.size,)
    assert np.array_equal(v.detach().cpu().numpy().astype(np.float64), want)
    assert np.array_equal(want, sr.sddmm_ref(rowptr, col, x, y))
    v.backward(torch.from_numpy(g).to(DEV))
    assert np.array_equal(xd.grad.cpu().numpy().astype(np.float64), want_gx)
    assert np.array_equal(yd.grad.cpu().numpy().astype(np.float64), want_gy)
    # the method form, without autograd, and on operands that start 4 bytes into an allocation
    base_x = torch.empty(M * K + 1, device=DEV)
    base_y = torch.empty(N * K + 1, device=DEV)
    xm, ym = base_x[1:].view(M, K), base_y[1:].view(N, K)
    xm.copy_(xd.detach())
    ym.copy_(yd.detach())
    assert torch.equal(A.sddmm(xm, ym).storage.value(), v.detach())


def test_sddmm_through_ops_without_a_csc_view():
    """ops.sddmm on bare (rowptr, col): the backward of y builds the CSC view itself."""
    from paddle_sparse_amd import ops

    rng = np.random.default_rng(43)
    lens = [0, 5, 130, 1, 0, 64]
    M, N, K = len(lens), 150, 8
    rowptr, col = pattern(rng, lens, N)
    x, y, g = ints(rng, (M, K), -4, 4), ints(rng, (N, K), -4, 4), ints(rng, col.size, -2, 2)
    want, want_gx, want_gy = dense_reference(rowptr, col, x, y, g)
    xd, yd = torch.from_numpy(x).to(DEV).requires_grad_(), torch.from_numpy(y).to(DEV).requires_grad_()
    out = ops.sddmm(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), xd, yd)
    out.backward(torch.from_numpy(g).to(DEV))
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64), want)
    assert np.array_equal(xd.grad.cpu().numpy().astype(np.float64), want_gx)
    assert np.array_equal(yd.grad.cpu().numpy().astype(np.float64), want_gy)


def test_sddmm_with_duplicate_entries_and_existing_values():
    """Duplicates are separate entries with the same score; the values `src` holds are not read."""
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(44)
    row = np.array([0, 0, 0, 1, 3, 3, 3, 3, 4], dtype=np.int64)
    col = np.array([1, 1, 6, 0, 2, 2, 2, 5, 6], dtype=np.int64)
    M, N, K = 5, 7, 3
    rowptr = np.searchsorted(row, np.arange(M + 1)).astype(np.int64)
    x, y, g = ints(rng, (M, K), -4, 4), ints(rng, (N, K), -4, 4), ints(rng, col.size, -2, 2)
    want, want_gx, want_gy = dense_reference(rowptr, col, x, y, g)
    A = psa.SparseTensor(row=torch.from_numpy(row).to(DEV), col=torch.from_numpy(col).to(DEV),
                         value=torch.full((col.size,), float("nan"), device=DEV), sparse_sizes=(M, N), is_sorted=True)
    xd, yd = torch.from_numpy(x).to(DEV).requires_grad_(), torch.from_numpy(y).to(DEV).requires_grad_()
    out = A.sddmm(xd, yd)
    assert out.nnz() == col.size
    v = out.storage.value()
    v.backward(torch.from_numpy(g).to(DEV))
    assert np.array_equal(v.detach().cpu().numpy().astype(np.float64), want)
    assert np.array_equal(xd.grad.cpu().numpy().astype(np.float64), want_gx)
    assert np.array_equal(yd.grad.cpu().numpy().astype(np.float64), want_gy)


def test_attention_step_exact():
    """softmax(sddmm(A, q, k), 1) @ v with identical rows in k: equal scores within a row, degrees that are
    powers of two, small integers everywhere.  Output, grad_v, grad_q (exactly 0) and grad_k equal dense
    float64 autograd bit for bit."""
    import paddle_sparse_amd as psa

    rng = np.random.default_rng(45)
    lens = [1, 2, 4, 8, 16, 32, 64, 128, 256, 0, 4, 2, 256, 1]
    M, N, K, F = len(lens), 300, 4, 8
    rowptr, col = pattern(rng, lens, N)
    row = np.repeat(np.arange(M), np.diff(rowptr))
    q = ints(rng, (M, K), -2, 2)
    k = np.tile(ints(rng, (1, K), -2, 2), (N, 1))
    v = ints(rng, (N, F), -2, 2)
    go = ints(rng, (M, F), -2, 2)

    qt, kt, vt = (torch.from_numpy(a.astype(np.float64)).requires_grad_() for a in (q, k, v))
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[torch.from_numpy(row), torch.from_numpy(col)] = True
    # missing entries at -inf; the row without entries at 0 instead, so that no NaN enters the dense backward
    fill = torch.where(mask.any(1, keepdim=True), torch.tensor(float("-inf"), dtype=torch.float64),
                       torch.tensor(0.0, dtype=torch.float64))
    scores = torch.where(mask, qt @ kt.T, fill.expand(M, N))
    att = torch.softmax(scores, dim=1)
    att = torch.where(mask, att, torch.zeros_like(att))
    (att @ vt).backward(torch.from_numpy(go.astype(np.float64)))
    want = (att @ vt).detach().numpy()

    A = psa.SparseTensor(rowptr=torch.from_numpy(rowptr).to(DEV), col=torch.from_numpy(col).to(DEV),
                         sparse_sizes=(M, N), is_sorted=True)
    qd, kd, vd = (torch.from_numpy(a).to(DEV).requires_grad_() for a in (q, k, v))
    out = psa.softmax(psa.sddmm(A, qd, kd), 1) @ vd
    out.backward(torch.from_numpy(go).to(DEV))
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64), want)
    assert np.array_equal(vd.grad.cpu().numpy().astype(np.float64), vt.grad.numpy())
    assert not qd.grad.cpu().numpy().any() and not qt.grad.numpy().any()
    assert np.array_equal(kd.grad.cpu().numpy().astype(np.float64), kt.grad.numpy())


def test_sddmm_errors():
    import paddle_sparse_amd as psa

    A = psa.SparseTensor(row=torch.tensor([0, 1], device=DEV), col=torch.tensor([1, 2], device=DEV), sparse_sizes=(2, 3))
    x, y = torch.zeros(2, 4, device=DEV), torch.zeros(3, 4, device=DEV)
    assert A.sddmm(x, y).storage.value().tolist() == [0.0, 0.0]
    with pytest.raises(RuntimeError):
        A.sddmm(x.cpu(), y)
    with pytest.raises(RuntimeError):
        A.sddmm(x, y.cpu())
    with pytest.raises(ValueError):
        A.sddmm(torch.zeros(3, 4, device=DEV), y)  # M
    with pytest.raises(ValueError):
        A.sddmm(x, torch.zeros(2, 4, device=DEV))  # N
    with pytest.raises(ValueError):
        A.sddmm(x, torch.zeros(3, 5, device=DEV))  # K
    with pytest.raises(ValueError):
        A.sddmm(torch.zeros(2, device=DEV), y)  # 1-D
    with pytest.raises(TypeError):
        A.sddmm(x.double(), y.double())
    with pytest.raises(TypeError):
        A.sddmm(x.half(), y)
    with pytest.raises(TypeError):
        A.sddmm(x, [[0.0]])
